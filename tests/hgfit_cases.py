"""Double Henyey-Greenstein fit of a phase function (Scatter_0.subfithgm :1948 -> mrqminl :2017 -> mrqcofl :2096 ->
subhgphas :2122 -> henyey :2159): the cases of tests/golden/hgfit.npz (tools/golden/gen_golden_hgfit.py runs the reference
on them) and `subfithgm_np`, the project's own NumPy restatement -- the written-down contract of k_hg_fit in
csrc/ansfm_hgfit_kernels.hip.h.

Per fit, a Levenberg-Marquardt chain on x = (f, g1, g2) from (0.5, 0.5, -0.5) against log(phase):
  * P(x) = f h(g1) + (1 - f) h(g2), h(g) = (1 - g g) / (1 + g g - 2 g cos(theta)) ** 1.5, at x and at the three points
    x_j + dx (dx = 0.01; -0.01 where f + dx > 0.99 or g1 + dx > 0.98), kk_j = (P_j - P) / dx / P, dy = log(phase) - log(P)
  * ten sums over the angles: alpha_jk = sum kk_j kk_k (j >= k), beta_j = sum dy kk_j, chisq = sum dy dy
  * (alpha with its diagonal times (1 + alamda)) da = beta; the trial point x + da clipped to f in [1e-6, 0.999999],
    g1 in [0, 0.98], g2 in [-0.98, -0.1] by comparisons (a NaN passes)
  * chisq_trial <= ochisq accepts (alamda * 0.9, x, alpha, beta taken from the trial), else alamda * 1.5, capped at 1e36
  * alamda starts at 1000; the chain ends after more than 5 accepted calls in a row with |chisq - prev| / (chisq + prev +
    1e-30) < 1e-8 (prev: chisq before the call, 0.0 before the first), or after 1000 calls
  * f, g1, g2, rms = sqrt(chisq)

order="reference": the sums run over the angles one after the other and the normal equations go through np.linalg.inv and
np.dot, as the reference's do: its call and accepted counts are reproduced.  order="kernel": the kernel's arithmetic -- the
angles i, i + 64, ... summed in ascending order per lane, the halving tree v[i] += v[i + s] (s = 32 .. 1) over the 64 lanes,
and Gaussian elimination with partial pivoting (solve3) on the 3 x 3 system; an exact zero pivot raises HgFitFailure.
cos, log and pow, which the device may round differently, can be replaced (`fn`, as in mie_cases.NUMPY_FUNCS).

The fits of a call are independent; the restatement steps all of them together, one array element per fit.

cases(golden_dir): name -> (theta, phase).  Phase functions the Mie goldens hold are taken from them (reference results);
the 41- and 129-angle ones are makephase_np's.  A test reads the inputs from tests/golden/hgfit.npz."""
import math
import os

import numpy as np

import mie_cases as mc

LANES = 64
NPHASE_CAP = 8192
NOVER = 1000
NUMPY_FUNCS = mc.NUMPY_FUNCS


class HgFitFailure(ValueError):
    """an exact zero pivot in the normal equations of a fit"""


shifted_funcs = mc.shifted_funcs         # every cos, log and pow result moved one ulp towards direction * inf


def _sum_reference(v):
    """sum over axis 0 one after the other"""
    return np.add.accumulate(v, axis=0)[-1]


def _sum_kernel(v):
    """sum over axis 0 as k_hg_fit does: lane l adds its angles l, l + 64, ... in ascending order, then the halving tree"""
    n = v.shape[0]
    npass = -(-n // LANES)
    pad = np.zeros((npass * LANES,) + v.shape[1:])
    pad[:n] = v
    lane = np.add.accumulate(pad.reshape((npass, LANES) + v.shape[1:]), axis=0)[-1]
    s = LANES // 2
    while s >= 1:
        lane[:s] = lane[:s] + lane[s:2 * s]
        s //= 2
    return lane[0]


def henyey_terms(calpha, g, pow_fn):
    """h(g) at every angle; calpha (nphase, 1), g (nfit,) -> (nphase, nfit)"""
    return (1.0 - g * g) / pow_fn(1.0 + g * g - 2 * g * calpha, 1.5)


_libm_pow = np.frompyfunc(math.pow, 2, 1)


def scalar_pow(a, b):
    """a ** b element by element through the C library, as a NumPy scalar's ** goes: NumPy's array power may round otherwise"""
    return _libm_pow(a, b).astype(np.float64)


def normal_sums(calpha, lphase, x, order, fn):
    """mrqcofl at x (nfit, 3): the ten sums -> a (nfit, 6) = alpha 00 10 11 20 21 22, b (nfit, 3), chisq (nfit,)"""
    f, g1, g2 = x[:, 0], x[:, 1], x[:, 2]
    # subhgphas: the perturbed points, with the sign flips
    ft = f + 0.01
    ft = np.where(ft > 0.99, f - 0.01, ft)
    g1t = g1 + 0.01
    g1t = np.where(g1t > 0.98, g1 - 0.01, g1t)
    g2t = g2 + 0.01
    dx0, dx1, dx2 = ft - f, g1t - g1, g2t - g2
    h1, h2 = henyey_terms(calpha, g1, fn.pow), henyey_terms(calpha, g2, fn.pow)
    cphase = f * h1 + (1.0 - f) * h2
    # the reference evaluates the perturbed points angle by angle (:2151-2152), where ** is the C library's pow, and the
    # unperturbed one on the array (:2136), where it is NumPy's; the kernel has one pow, and h(g1), h(g2) once
    if order == "reference" and fn is NUMPY_FUNCS:
        s1, s2 = henyey_terms(calpha, g1, scalar_pow), henyey_terms(calpha, g2, scalar_pow)
        h1t, h2t = henyey_terms(calpha, g1t, scalar_pow), henyey_terms(calpha, g2t, scalar_pow)
    else:
        s1, s2 = h1, h2
        h1t, h2t = henyey_terms(calpha, g1t, fn.pow), henyey_terms(calpha, g2t, fn.pow)
    k0 = ((ft * s1 + (1.0 - ft) * s2) - cphase) / dx0
    k1 = ((f * h1t + (1.0 - f) * s2) - cphase) / dx1
    k2 = ((f * s1 + (1.0 - f) * h2t) - cphase) / dx2
    k0, k1, k2 = k0 / cphase, k1 / cphase, k2 / cphase
    dy = lphase - fn.log(cphase)
    terms = np.stack([k0 * k0, k1 * k0, k1 * k1, k2 * k0, k2 * k1, k2 * k2, dy * k0, dy * k1, dy * k2, dy * dy], axis=0)
    tot = np.stack([(_sum_kernel if order == "kernel" else _sum_reference)(t) for t in terms], axis=1)
    return tot[:, :6], tot[:, 6:9], tot[:, 9]


def solve3(a, lam, b):
    """k_hg_fit's elimination: (alpha with diagonal (1 + lam)) da = b for every fit; a (n, 6), lam (n,), b (n, 3) ->
    da (n, 3), failed (n,) bool.  Column by column the row with the largest magnitude becomes the pivot (the first of equals,
    a NaN never displaces); an exact zero pivot fails the fit."""
    with np.errstate(all="ignore"):
        return _solve3(a, lam, b)


def _solve3(a, lam, b):
    n = a.shape[0]
    M = np.empty((n, 3, 3))
    M[:, 0, 0] = a[:, 0] * (1.0 + lam); M[:, 1, 1] = a[:, 2] * (1.0 + lam); M[:, 2, 2] = a[:, 5] * (1.0 + lam)
    M[:, 1, 0] = M[:, 0, 1] = a[:, 1]; M[:, 2, 0] = M[:, 0, 2] = a[:, 3]; M[:, 2, 1] = M[:, 1, 2] = a[:, 4]
    r = b.copy()
    idx = np.arange(n)

    def swap(i, j, where):
        for arr in (M, r):
            t = arr[idx, i].copy()
            arr[idx, i] = np.where(where[(...,) + (None,) * (arr.ndim - 2)], arr[idx, j], arr[idx, i])
            arr[idx, j] = np.where(where[(...,) + (None,) * (arr.ndim - 2)], t, arr[idx, j])

    big = np.abs(M[:, 0, 0])
    p1 = np.abs(M[:, 1, 0]) > big
    big = np.where(p1, np.abs(M[:, 1, 0]), big)
    p2 = np.abs(M[:, 2, 0]) > big
    swap(0, 1, p1 & ~p2)
    swap(0, 2, p2)
    failed = M[:, 0, 0] == 0.0
    for i in (1, 2):
        l = M[:, i, 0] / M[:, 0, 0]
        M[:, i, 1] = M[:, i, 1] - l * M[:, 0, 1]
        M[:, i, 2] = M[:, i, 2] - l * M[:, 0, 2]
        r[:, i] = r[:, i] - l * r[:, 0]
    swap(1, 2, np.abs(M[:, 2, 1]) > np.abs(M[:, 1, 1]))
    failed = failed | (M[:, 1, 1] == 0.0)
    l = M[:, 2, 1] / M[:, 1, 1]
    M[:, 2, 2] = M[:, 2, 2] - l * M[:, 1, 2]
    r[:, 2] = r[:, 2] - l * r[:, 1]
    failed = failed | (M[:, 2, 2] == 0.0)
    d2 = r[:, 2] / M[:, 2, 2]
    d1 = (r[:, 1] - M[:, 1, 2] * d2) / M[:, 1, 1]
    d0 = (r[:, 0] - M[:, 0, 1] * d1 - M[:, 0, 2] * d2) / M[:, 0, 0]
    return np.stack([d0, d1, d2], axis=1), failed


def _solve_reference(a, lam, b):
    """mrqminl's own way (:2036-2047): np.linalg.inv, then np.dot, fit by fit"""
    da = np.empty_like(b)
    for i in range(a.shape[0]):
        covar = np.array([[a[i, 0] * (1.0 + lam[i]), a[i, 1], a[i, 3]],
                          [a[i, 1], a[i, 2] * (1.0 + lam[i]), a[i, 4]],
                          [a[i, 3], a[i, 4], a[i, 5] * (1.0 + lam[i])]])
        da[i] = np.dot(np.ascontiguousarray(np.linalg.inv(covar)), np.ascontiguousarray(b[i]))
    return da


def clip_trial(xt):
    """the reference's comparisons (:2055-2070); a NaN passes through"""
    f, g1, g2 = xt[:, 0].copy(), xt[:, 1].copy(), xt[:, 2].copy()
    f[f > 0.999999] = 0.999999
    f[f < 0.000001] = 0.000001
    g1[g1 > 0.98] = 0.98
    g1[g1 < 0.0] = 0.0
    g2[g2 < -0.98] = -0.98
    g2[g2 > -0.1] = -0.1
    return np.stack([f, g1, g2], axis=1)


def subfithgm_np(theta, phase, order="reference", fn=NUMPY_FUNCS, return_counts=False):
    """(f, g1, g2, rms[, counts (nfit, 2) = calls of mrqminl, accepted ones]) of Scatter_0.subfithgm(theta, phase)"""
    assert order in ("reference", "kernel")
    theta = np.asarray(theta, dtype=np.float64)
    phase = np.asarray(phase, dtype=np.float64)
    nfit, nphase = phase.shape
    assert theta.shape == (nphase,) and 1 <= nphase <= NPHASE_CAP
    with np.errstate(all="ignore"):
        calpha = fn.cos(theta * np.pi / 180.0)[:, None]
        lphase = fn.log(phase).T                          # (nphase, nfit)
        x = np.tile(np.array([0.5, 0.5, -0.5]), (nfit, 1))
        alpha, beta, chisq0 = normal_sums(calpha, lphase, x, order, fn)
        ochisq = chisq0.copy()
        chisq = np.zeros(nfit)                            # what prev_chisq sees before the first call
        alamda = np.full(nfit, 1000.0)
        nc = np.zeros(nfit, dtype=np.int64)
        counts = np.zeros((nfit, 2), dtype=np.int32)
        active = np.ones(nfit, dtype=bool)
        for it in range(NOVER):
            k = np.flatnonzero(active)
            if k.shape[0] == 0:
                break
            prev = chisq[k]
            if order == "kernel":
                da, failed = solve3(alpha[k], alamda[k], beta[k])
                if failed.any():
                    raise HgFitFailure("hg_fit: fit %d: the normal equations have a zero pivot" % k[np.argmax(failed)])
            else:
                da = _solve_reference(alpha[k], alamda[k], beta[k])
            xt = clip_trial(x[k] + da)
            a_new, b_new, c_new = normal_sums(calpha, lphase[:, k], xt, order, fn)
            acc = c_new <= ochisq[k]
            ka = k[acc]
            alamda[k] = np.where(acc, 0.9 * alamda[k], np.minimum(1.5 * alamda[k], 1e36))
            x[ka], alpha[ka], beta[ka] = xt[acc], a_new[acc], b_new[acc]
            ochisq[ka] = c_new[acc]
            chisq[k] = ochisq[k]
            counts[k, 0] += 1
            counts[ka, 1] += 1
            rel = np.abs(chisq[ka] - prev[acc]) / (chisq[ka] + prev[acc] + 1e-30)
            nc[ka] = np.where(rel < 1e-8, nc[ka] + 1, 0)
            active[ka[nc[ka] > 5]] = False
        out = (x[:, 0].copy(), x[:, 1].copy(), x[:, 2].copy(), np.sqrt(chisq))
    return out + (counts,) if return_counts else out


def deviations(got, ref):
    """(parameters, rms): the largest relative deviations of (f, g1, g2) and of rms from a reference result.  Where the
    reference's value is 0 (g1 on its clip), not finite or NaN (`zero-phase`), equality is asked for: the deviation is 0 when the
    values are the same, inf otherwise."""
    def rel(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        with np.errstate(all="ignore"):
            d = np.abs(a - b) / np.abs(b)
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        exact = (b == 0.0) | ~np.isfinite(b)
        d = np.where(exact, np.where(same, 0.0, np.inf), d)
        return float(np.max(np.where(np.isnan(d), np.inf, d)))
    return max(rel(got[i], ref[i]) for i in range(3)), rel(got[3], ref[3])


CASE_NAMES = ("lognormal-41", "single-41", "small-41", "gamma-6", "nphase-1", "nphase-2", "nphase-65", "nphase-66", "nphase-129",
              "fits-130", "zero-phase")
# the fits taken from the Mie goldens: case -> (file, case there)
FROM_MIE = {"gamma-6": ("mie.npz", "gamma-open-no90"), "nphase-2": ("mie_edges.npz", "x2000-single"),
            "nphase-65": ("mie_edges.npz", "theta-33-90"), "nphase-66": ("mie_edges.npz", "theta-33"),
            "fits-130": ("mie_edges.npz", "ws-halved")}
THETA21 = np.linspace(0.0, 90.0, 21)                        # the default 41 angles out to 180 degrees
ZERO_AT = 20                                                # the angle of `zero-phase` whose phase function is an exact 0


def computed_inputs():
    """the Mie inputs of the cases no golden holds: makephase_np's arguments"""
    even = mc.edge_cases()["theta-0"]
    return {
        "lognormal-41": mc._case([0.8, 2.0, 5.0, 10.0], 2, (0.5, 0.3), (0.05, 3.05, 0.05), (1.4, 0.01), THETA21),
        "single-41": mc._case([0.5], 4, (3.0,), (3.0, 3.0, 3.0), (1.33, 0.001), THETA21),          # x = 37.7
        "small-41": mc._case([10.0], 4, (0.05,), (0.05, 0.05, 0.05), (1.4, 0.01), THETA21),        # x = 0.0314
        "nphase-129": dict(even, theta=np.linspace(0.0, 90.0, 65)),
    }


def cases(golden_dir):
    """name -> (theta (nphase,), phase (nfit, nphase)), built from the Mie goldens and the restatement of the Mie kernels"""
    out = {}
    files = {}
    for name in CASE_NAMES:
        if name in FROM_MIE:
            fname, src = FROM_MIE[name]
            g = files.setdefault(fname, mc.load_golden(os.path.join(golden_dir, fname)))[src]
            out[name] = (g["thetax"].copy(), g["phas"].copy())
    # 0 and 180 degrees of the sphere at x = 2011, whose forward peak of 3.8e6 no clipped (f, g1) reaches: two angles, and then
    # the forward one alone, leave alpha rank-deficient, and the residual stays far above its rounding (a phase function
    # that one or two angles fit exactly ends at rms = 0 or 2e-16, of which no digit is defined)
    out["nphase-2"] = (out["nphase-2"][0][[0, 6]].copy(), out["nphase-2"][1][:, [0, 6]].copy())
    # 64 wavelengths x 5 angles twice, the second time 1.25 times as large, and two more: 130 different fits.  (The 130
    # wavelengths of `waves-130` are not used: the 1e-8 of the stopping rule moves 58 of them by 2e-9 to 1.7e-8.)
    theta, phase = out["fits-130"]
    out["fits-130"] = (theta, np.concatenate([phase, 1.25 * phase, 0.8 * phase[:2]], axis=0))
    for name, d in computed_inputs().items():
        _, _, thetax, phas = mc.makephase_np(d["wavel"], d["iscat"], d["dsize"], d["rs"], d["refindx"], d["theta"])
        out[name] = (thetax, phas)
    out["nphase-1"] = (out["nphase-2"][0][:1].copy(), out["nphase-2"][1][:, :1].copy())
    theta, phase = out["lognormal-41"]
    zero = phase[:1].copy()
    zero[0, ZERO_AT] = 0.0
    out["zero-phase"] = (theta.copy(), zero)
    return {name: out[name] for name in CASE_NAMES}


def singular_case(golden_dir):
    """(theta, phase) of `singular-90`, the one angle of the Mie golden `theta-90`: at 90 degrees h(0.5) = h(-0.5) bit for bit,
    so the start point's derivative with respect to f is an exact 0 and with it a row of alpha.  The reference ends in
    np.linalg.inv's "Singular matrix"; the kernel's elimination meets the zero pivot and flags the fit."""
    g = mc.load_golden(os.path.join(golden_dir, "mie_edges.npz"))["theta-90"]
    return g["thetax"].copy(), g["phas"].copy()


def load_golden(path):
    z = np.load(path)
    out = {}
    for key in z.files:
        name, field = key.split("__")
        out.setdefault(name, {})[field] = z[key]
    return out
