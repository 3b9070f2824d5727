"""Mie theory over a size distribution (Scatter_0.makephase :1828 -> miescat :1600 -> dmie :1399): the cases of
tests/golden/mie.npz (tools/golden/gen_golden_mie.py runs the reference on them) and `makephase_np`, the project's own
NumPy restatement -- the written-down contract of the kernels in csrc/ansfm_mie_kernels.hip.h.

Per (wavelength, radius), x = 2 pi r / lambda, m = n_r - i n_i, z = m x:
  * D_n(z), the logarithmic derivative of the Riccati-Bessel function psi_n, downwards from D = 0 at
    nmx1 + 1, nmx1 = max(150, int(1.1 |m| x)):  D_n = (n + 1)/z - 1 / ((n + 1)/z + D_{n+1})
  * xi_n = psi_n + i chi_n upwards from xi_{-1} = (cos x, -sin x), xi_0 = (sin x, cos x):
    xi_n = (2n - 1)/x xi_{n-1} - xi_{n-2}
  * a_n = ((D_n/m + n/x) psi_n - psi_{n-1}) / ((D_n/m + n/x) xi_n - xi_{n-1}), b_n the same with D_n m
  * the series ends with the first n >= 2 whose |a_n|^2 + |b_n|^2 < 1e-14; needing more than
    nmx2 = max(135, int(|m| x)) terms, or nmx1 >= 29999, is a failure
  * Q_ext = 2/x^2 sum (2n + 1) Re(a_n + b_n), Q_sca = 2/x^2 sum (2n + 1)(|a_n|^2 + |b_n|^2)
  * amplitudes with pi_n, tau_n (pi_0 = 0, pi_1 = 1, tau_1 = cos): S_a = sum (2n+1)/(n(n+1)) (a_n pi_n + b_n tau_n),
    S_b the same with a and b exchanged; at 180 - theta pi_n carries (-1)^(n+1) and tau_n (-1)^n;
    f = (|S_a|^2 + |S_b|^2)/2 = (M1 + M2)/2
Over radii r_m = rs[0] + m rs[2] with Simpson weights (1, 4, 2, 4, ... ; the last radius of a closed range 1) / 3 and the
distribution n(r): k_sca = sum pi r^2 Q_sca n w, k_ext likewise, norm = sum n w, phase = lambda^2 sum f n w / (pi k_sca).
A closed range (rs[1] >= rs[0]) has 1 + int((rs[1] - rs[0])/rs[2]) radii, one more when that is odd and above 1.  An
open range ends with -- and includes -- the first radius with r >= r_peak and n Q_sca <= 1e-6 max_so_far(n Q_sca).

The order of every operation is the reference's, so that the restatement differs from it by the complex divisions
(Python's form in places, NumPy's here) and the order of the sum over radii only.  chunk_order=True sums the radii as the
kernels do: chunks of 64 radii aligned at m = 0, inside a chunk the halving tree v[i] += v[i + s] (s = 32 ... 1), the
chunks' sums then added in ascending order.

edge_cases() (tests/golden/mie_edges.npz) enters what the eight golden cases leave out:
  perwave-m, waves-130     a refractive index per wavelength; 130 wavelengths are three blocks of k_mie_cutoff
  nmx150                   50 radii over which 1.1 |m| x runs from 145 to 155, across nmx1's switch at 150
  x2000-single             x = 2011: D_n downwards from 2940
  absorbing                m = 2 - 3i and 0.3 - 4i
  small-x                  10 radii at x from 3.0e-3 to 3.0e-2, where the upward recurrence cancels
  fail-behind-cut          an open range that ends after 26 radii, with series that fail from radius 93 on in the same block
  closed-2                 both Simpson end weights side by side
  theta-0, theta-90, theta-33, theta-33-90      1 and 33 angles, with and without 90 degrees
  open-64, -65, -128, -129 open ranges that end on the last radius of a chunk or block, and on the first of the next
  ws-halved                64 wavelengths x 300 radii at x up to 829: the 1 GiB workspace bound halves the block of radii
The elementary functions the device may round differently (sin, cos, exp, log, pow) can be replaced (`fn`), and
one_ulp_sensitivity(case) measures how strongly a case amplifies one ulp in them: about 2e-14 / x^2 at small x."""
import types

import numpy as np

INPUTS = ("wavel", "iscat", "dsize", "rs", "refindx", "theta")
CHUNK = 64
RADIUS_CAP = 1 << 20

# the elementary functions of the restatement: what the device is free to round differently.  `pow` is
# the operator, whose squares and identities NumPy takes without the library's pow.
NUMPY_FUNCS = types.SimpleNamespace(sin=np.sin, cos=np.cos, exp=np.exp, log=np.log, pow=lambda a, b: a ** b)


def shifted_funcs(direction):
    """the elementary functions with every cos, exp, log and pow result moved one ulp towards direction * inf and every sin
    result one ulp the other way"""
    to = lambda f, d: (lambda *a: np.nextafter(f(*a), d * np.inf))
    n = NUMPY_FUNCS
    return types.SimpleNamespace(sin=to(n.sin, -direction), cos=to(n.cos, direction), exp=to(n.exp, direction),
                                 log=to(n.log, direction), pow=to(n.pow, direction))


class MieFailure(ValueError):
    """one of the reference's two give-ups, or an open range that does not end"""


def nphas_of(theta):
    theta = np.asarray(theta, dtype=np.float64)
    return 2 * theta.shape[0] - 1 if np.count_nonzero(theta == 90.0) == 1 else 2 * theta.shape[0]


def thetax_of(theta):
    theta = np.asarray(theta, dtype=np.float64)
    nphas = nphas_of(theta)
    out = np.zeros(nphas)
    out[:theta.shape[0]] = theta
    for i in range(theta.shape[0], nphas):
        out[i] = 180.0 - out[nphas - i - 1]
    return out


def radius_count(rs):
    """radii of a closed range; None for an open one"""
    if rs[1] < rs[0]:
        return None
    inr = 1 + int((rs[1] - rs[0]) / rs[2])
    if inr > 1 and inr % 2 != 0:
        inr += 1
    return inr


def peak_radius(iscat, dsize, fn=NUMPY_FUNCS):
    """r_peak of the open range's test (:1693-1709)"""
    if dsize[1] == 0:
        return 0.0
    aa, bb = dsize[0], dsize[1]
    if iscat == 1:
        return dsize[2] * aa * bb
    if iscat == 2:
        return fn.exp(fn.log(aa) - bb ** 2)
    if iscat == 3:
        return fn.pow(aa / (bb * dsize[2]), 1.0 / dsize[2])
    return 0.0


def size_weight(iscat, dsize, rr, fn=NUMPY_FUNCS):
    """n(r) (:1758-1773)"""
    if dsize[1] == 0 or iscat == 4:
        return np.ones_like(rr)
    aa, bb = dsize[0], dsize[1]
    if iscat == 1:
        return fn.pow(rr, dsize[2]) * fn.exp(-rr / (aa * bb))
    if iscat == 2:
        return 1. / (rr * bb * np.sqrt(2 * np.pi)) * fn.exp(-(fn.log(rr) - fn.log(aa)) ** 2. / (2. * bb ** 2.))
    return fn.pow(rr, aa) * fn.exp(-bb * fn.pow(rr, dsize[2]))


def simpson_weight(m, inr, delr):
    """(:1786-1791); inr = None for an open range"""
    vv = np.where(m % 2 == 0, 2.0 * delr / 3.0, 4.0 * delr / 3.0)
    last = -1 if inr is None else inr - 1
    return np.where((m == 0) | (m == last), delr / 3.0, vv)


def mie_terms(x, rfr, rfi, cstht, si2tht, fn=NUMPY_FUNCS):
    """dmie for an array of size parameters: Q_ext, Q_sca, the term counts, f at theta and at 180 - theta (R, A), and the
    failure codes (0; 1: nmx1 >= 29999; 2: more than nmx2 terms)"""
    R, A = x.shape[0], cstht.shape[0]
    rf = complex(rfr, -rfi)
    rrf = 1.0 / np.complex128(rf)
    rx = 1.0 / x
    rrfx = rrf * rx
    t0 = np.sqrt(x * x * (rfr * rfr + rfi * rfi))
    nmx1 = (1.1 * t0).astype(np.int64)
    nmx2 = t0.astype(np.int64)
    fail = np.where(nmx1 < 29999, 0, 1)
    small = ~(nmx1 > 150)
    nmx1 = np.where(small, 150, nmx1); nmx2 = np.where(small, 135, nmx2)
    nmx1 = np.where(fail == 1, 150, nmx1); nmx2 = np.where(fail == 1, 135, nmx2)       # nothing of a failed radius is used
    nstore = int(nmx2.max())
    D = np.zeros((nstore + 1, R), dtype=np.complex128)
    cur = np.zeros(R, dtype=np.complex128)
    for nn in range(int(nmx1.max()), 0, -1):
        new = (nn + 1) * rrfx - 1.0 / ((nn + 1) * rrfx + cur)
        cur = np.where(nn <= nmx1, new, 0.0)
        if nn <= nstore:
            D[nn] = cur
    cx, sx = fn.cos(x), fn.sin(x)
    wm1 = cx - 1j * sx
    wfn1 = sx + 1j * cx
    wfn2 = rx * wfn1 - wm1
    tc1 = D[1] * rrf + rx
    tc2 = D[1] * rf + rx
    fna = (tc1 * wfn2.real - wfn1.real) / (tc1 * wfn2 - wfn1)
    fnb = (tc2 * wfn2.real - wfn1.real) / (tc2 * wfn2 - wfn1)
    tb0, tb1, tc0, tc1i = 1.5 * fna.real, 1.5 * fna.imag, 1.5 * fnb.real, 1.5 * fnb.imag
    pi0, pi1 = np.zeros(A), np.ones(A)
    tau0, tau1 = np.zeros(A), cstht.copy()
    col = lambda v: v[:, None]
    ef = [col(tb0) * pi1 + col(tc0) * tau1, col(tb1) * pi1 + col(tc1i) * tau1,
          col(tc0) * pi1 + col(tb0) * tau1, col(tc1i) * pi1 + col(tb1) * tau1]
    eb = [col(tb0) * pi1 - col(tc0) * tau1, col(tb1) * pi1 - col(tc1i) * tau1,
          col(tc0) * pi1 - col(tb0) * tau1, col(tc1i) * pi1 - col(tb1) * tau1]
    qext = 2.0 * (tb0 + tc0)
    qscat = (tb0 ** 2 + tb1 ** 2 + tc0 ** 2 + tc1i ** 2) / 0.75
    nterm = np.ones(R, dtype=np.int64)
    active = fail == 0
    n = 2
    while active.any():
        u0, u1, u2 = float(2 * n - 1), float(n - 1), float(2 * n + 1)
        pi2 = (u0 * pi1 * cstht - n * pi0) / u1
        tau2 = cstht * (pi2 - pi0) - u0 * si2tht * pi1 + tau0
        wm1 = wfn1; wfn1 = wfn2
        Dn = D[min(n, nstore)]
        tc1 = Dn * rrf + n * rx
        tc2 = Dn * rf + n * rx
        with np.errstate(all="ignore"):               # radii that have ended keep running here, unused
            wfn2 = u0 * rx * wfn1 - wm1
            fna = (tc1 * wfn2.real - wfn1.real) / (tc1 * wfn2 - wfn1)
            fnb = (tc2 * wfn2.real - wfn1.real) / (tc2 * wfn2 - wfn1)
            tb0, tb1, tc0, tc1i = fna.real, fna.imag, fnb.real, fnb.imag
            qext = np.where(active, qext + u2 * (tb0 + tc0), qext)
            t3 = tb0 ** 2 + tc0 ** 2 + tb1 ** 2 + tc1i ** 2
            qscat = np.where(active, qscat + u2 * t3, qscat)
            w = u2 / float(n * (n + 1))
            a2 = active[:, None]
            add = [w * (col(tb0) * pi2 + col(tc0) * tau2), w * (col(tb1) * pi2 + col(tc1i) * tau2),
                   w * (col(tc0) * pi2 + col(tb0) * tau2), w * (col(tc1i) * pi2 + col(tb1) * tau2)]
            if n % 2 == 0:
                sub = [w * (-col(tb0) * pi2 + col(tc0) * tau2), w * (-col(tb1) * pi2 + col(tc1i) * tau2),
                       w * (-col(tc0) * pi2 + col(tb0) * tau2), w * (-col(tc1i) * pi2 + col(tb1) * tau2)]
            else:
                sub = [w * (col(tb0) * pi2 - col(tc0) * tau2), w * (col(tb1) * pi2 - col(tc1i) * tau2),
                       w * (col(tc0) * pi2 - col(tb0) * tau2), w * (col(tc1i) * pi2 - col(tb1) * tau2)]
            for i in range(4):
                ef[i] = np.where(a2, ef[i] + add[i], ef[i])
                eb[i] = np.where(a2, eb[i] + sub[i], eb[i])
        nterm = np.where(active, n, nterm)
        ended = active & (t3 < 1e-14)
        active = active & ~ended
        n += 1
        pi0, pi1, tau0, tau1 = pi1, pi2, tau1, tau2
        over = active & (n > nmx2)
        fail = np.where(over, 2, fail)
        active = active & ~over
    f_fwd = (ef[2] ** 2 + ef[3] ** 2) + (ef[0] ** 2 + ef[1] ** 2)
    f_bwd = (eb[2] ** 2 + eb[3] ** 2) + (eb[0] ** 2 + eb[1] ** 2)
    t = 2.0 * rx * rx
    return qext * t, qscat * t, nterm, f_fwd, f_bwd, fail


def _ordered_sum(rows, chunk_order):
    """sum over axis 0: one after the other like the reference, or in the kernels' chunk order"""
    if not chunk_order:
        acc = np.zeros(rows.shape[1:])
        for r in rows:
            acc = acc + r
        return acc
    n = rows.shape[0]
    nch = -(-n // CHUNK)
    pad = np.zeros((nch * CHUNK,) + rows.shape[1:])
    pad[:n] = rows
    v = pad.reshape((nch, CHUNK) + rows.shape[1:]).copy()
    s = CHUNK // 2
    while s >= 1:
        v[:, :s] = v[:, :s] + v[:, s:2 * s]
        s //= 2
    acc = np.zeros(rows.shape[1:])
    for c in range(nch):
        acc = acc + v[c, 0]
    return acc


def miescat_np(xlam, iscat, dsize, rs, refindx, theta, chunk_order=False, block=256, cap=RADIUS_CAP, details=None,
               fn=NUMPY_FUNCS, memo=None):
    """memo: a dict that keeps mie_terms' results per block of radii, for a second call with the other order of the sum"""
    theta = np.asarray(theta, dtype=np.float64)
    A = theta.shape[0]
    nphas = nphas_of(theta)
    cstht = np.where(theta == 0.0, 1.0, np.where(theta == 90.0, 0.0, np.cos(np.pi * theta / 180.0)))
    si2tht = np.where(theta == 0.0, 0.0, np.where(theta == 90.0, 1.0, 1.0 - cstht * cstht))
    r1, delr = rs[0], rs[2]
    inr = radius_count(rs)
    rmax = peak_radius(iscat, dsize, fn) if inr is None else 0.0
    nqmax, m0, mcut = 0.0, 0, None
    rows_f, rows_k, ratios = [], [], []
    while mcut is None:
        if m0 >= cap:
            raise MieFailure("size integration did not terminate within %d radii (wavelength %g um)" % (cap, xlam))
        m = np.arange(m0, min(m0 + block, cap) if inr is None else min(m0 + block, inr), dtype=np.int64)
        rr = r1 + m * delr
        xx = 2.0 * np.pi * rr / xlam
        terms = None if memo is None else memo.get(m0)
        if terms is None:
            terms = mie_terms(xx, refindx[0], refindx[1], cstht, si2tht, fn)
            if memo is not None:
                memo[m0] = terms
        qext, qscat, nterm, f_fwd, f_bwd, fail = terms
        anr = size_weight(iscat, dsize, rr, fn)
        nq = anr * qscat
        last = m.shape[0] - 1
        for j in range(m.shape[0]):
            if fail[j]:
                raise MieFailure("Mie series failed (code %d) at wavelength %g um, radius %g um (index %d)"
                                 % (fail[j], xlam, rr[j], m[j]))
            nqmax = max(nqmax, nq[j])
            if inr is None:
                ratios.append(nq[j] / (1e-06 * nqmax) if rr[j] >= rmax else np.inf)
                if not (rr[j] < rmax or nq[j] > 1e-06 * nqmax):
                    mcut, last = int(m[j]), j
                    break
            elif m[j] == inr - 1:
                mcut = int(m[j])
        k = slice(0, last + 1)
        vv = simpson_weight(m[k], inr, delr)
        w = anr[k] * vv
        f = np.concatenate([f_fwd[k], f_bwd[k]], axis=1)
        rows_f.append(0.5 * anr[k, None] * vv[:, None] * f)
        rows_k.append(np.stack([np.pi * rr[k] * rr[k] * qscat[k] * anr[k] * vv, np.pi * rr[k] * rr[k] * qext[k] * anr[k] * vv,
                                w], axis=1))
        m0 += block
    if details is not None and inr is None:      # n Q_sca / (1e-6 max) at the last radius and the one before (inf below r_peak)
        details["ratio_end"], details["ratio_before"] = ratios[-1], (ratios[-2] if len(ratios) > 1 else np.inf)
    sf = _ordered_sum(np.concatenate(rows_f), chunk_order)
    kscat, kext, anorm = _ordered_sum(np.concatenate(rows_k), chunk_order)
    if anorm > 0.0:
        xscat, xext = kscat / anorm * 1e-08, kext / anorm * 1e-08
    else:
        xscat, xext, kscat = 0.0, 0.0, 1.0
    phas = np.zeros(nphas)
    for j in range(nphas):
        s = sf[j] if j < A else sf[A + (nphas - 1 - j)]
        phas[j] = xlam * xlam * (s / (np.pi * kscat))
    return xscat, xext, phas, mcut + 1


def makephase_np(wavel, iscat, dsize, rs, refindx, theta, chunk_order=False, return_counts=False, cap=RADIUS_CAP, details=None,
                 fn=NUMPY_FUNCS, memo=None):
    """(xscat, xext, thetax, phas[, n_radii]) of Scatter_0.makephase for iscat 1 .. 4, phas as miescat returns it (before the
    class method divides by 4 pi)"""
    wavel = np.atleast_1d(np.asarray(wavel, dtype=np.float64))
    theta = np.asarray(theta, dtype=np.float64)
    dsize = np.asarray(dsize, dtype=np.float64); rs = np.asarray(rs, dtype=np.float64)
    refindx = np.asarray(refindx, dtype=np.float64).reshape(wavel.shape[0], 2)
    if int(iscat) not in (1, 2, 3, 4):
        raise ValueError("iscat %d is not a Mie case" % iscat)
    if np.any(theta < 0.0) or np.any(theta > 90.0):
        raise ValueError("scattering angle outside [0, 90]")
    nw = wavel.shape[0]
    xscat, xext, counts = np.zeros(nw), np.zeros(nw), np.zeros(nw, dtype=np.int32)
    phas = np.zeros((nw, nphas_of(theta)))
    for i in range(nw):
        d = {} if details is not None else None
        xscat[i], xext[i], phas[i], counts[i] = miescat_np(wavel[i], int(iscat), dsize, rs, refindx[i], theta, chunk_order,
                                                           cap=cap, details=d, fn=fn,
                                                           memo=None if memo is None else memo.setdefault(i, {}))
        if details is not None:
            details.setdefault("per_wave", []).append(d)
    out = (xscat, xext, thetax_of(theta), phas)
    return out + (counts,) if return_counts else out


def _case(wavel, iscat, dsize, rs, m, theta):
    wavel = np.asarray(wavel, dtype=np.float64)
    d3 = np.zeros(3); d3[:len(dsize)] = dsize
    m = np.asarray(m, dtype=np.float64)
    refindx = np.tile(m, (wavel.shape[0], 1)) if m.ndim == 1 else m.reshape(wavel.shape[0], 2).copy()
    if rs is None:
        rs = (0.015 * wavel.min(), 0.0, 0.015 * wavel.min())
    return dict(wavel=wavel, iscat=np.int64(iscat), dsize=d3, rs=np.asarray(rs, dtype=np.float64), refindx=refindx,
                theta=np.asarray(theta, dtype=np.float64))


def golden_cases():
    """name -> inputs.  The closed ranges start at r = 0.05 um with step 0.02 um: (rs[1] - rs[0]) / rs[2] is kept a quarter
    step away from an integer so that the count does not rest on the rounding of the division."""
    closed = lambda n_before_bump: (0.05, 0.05 + (n_before_bump - 1 + 0.25) * 0.02, 0.02)
    return {
        "lognormal-open-90": _case([0.8, 2.0, 5.0], 2, (0.5, 0.3), None, (1.4, 0.01), [0.0, 10.0, 45.0, 90.0]),
        "gamma-open-no90": _case([1.0, 3.0], 1, (1.0, 0.1, 7.0), None, (1.33, 0.0), [5.0, 30.0, 60.0]),
        "mcs-open": _case([1.0, 2.0], 3, (2.0, 3.0, 1.0), None, (1.4, 0.01), [0.0, 20.0, 90.0]),
        "closed-even": _case([1.0], 2, (0.3, 0.4), closed(10), (1.5, 0.1), [0.0, 90.0]),          # 10 radii
        "closed-bumped": _case([1.0], 2, (0.3, 0.4), closed(11), (1.5, 0.1), [0.0, 90.0]),        # 11 -> 12 radii
        "closed-64": _case([1.0, 2.5], 2, (0.3, 0.4), closed(64), (1.5, 0.1), [0.0, 30.0, 90.0]),
        "closed-65": _case([1.0, 2.5], 2, (0.3, 0.4), closed(65), (1.5, 0.1), [0.0, 30.0, 90.0]),  # 65 -> 66 radii: two chunks
        "big-x-single": _case([0.5], 4, (10.0,), (10.0, 10.0, 10.0), (1.33, 0.001), [0.0, 30.0, 60.0, 90.0]),
    }


EXPECTED_RADII = {"closed-even": 10, "closed-bumped": 12, "closed-64": 64, "closed-65": 66, "big-x-single": 1}
OPEN_CASES = ("lognormal-open-90", "gamma-open-no90", "mcs-open")

# steps of the open ranges that end on the last radius of a chunk or block and on the first radius of the next
OPEN_STEPS = {"open-64": 0.03317858929464732, "open-65": 0.03267233616808404,
              "open-128": 0.01658729364682341, "open-129": 0.01647223611805903}


def edge_cases():
    """name -> inputs of tests/golden/mie_edges.npz: the paths of the kernels that golden_cases() does not enter."""
    closed = lambda n_before_bump, r0=0.05, step=0.02: (r0, r0 + (n_before_bump - 1 + 0.25) * step, step)
    even = dict(wavel=[1.0], iscat=2, dsize=(0.3, 0.4), rs=closed(10), m=(1.5, 0.1))       # the inputs of closed-even
    theta33 = np.linspace(0.0, 88.0, 33)
    w130, w64 = np.linspace(0.8, 5.0, 130), np.linspace(0.5, 0.6, 64)
    cases = {
        # a refractive index per wavelength (model 444 retrieves this array)
        "perwave-m": _case([0.8, 2.0, 5.0], 2, (0.5, 0.3), (0.012, 0.0, 0.012), [[1.4, 0.01], [1.33, 0.0], [1.8, 0.5]],
                           [0.0, 10.0, 45.0, 90.0]),
        # 1.1 |m| x from 145 to 155: nmx1 switches from the floor of 150 to int(1.1 |m| x) inside the range
        "nmx150": _case([1.0], 4, (14.0,), closed(50, 14.0), (1.5, 0.0), [0.0, 30.0, 60.0, 90.0]),
        # x = 2011: D_n downwards from 2940, 2675 workspace rows
        "x2000-single": _case([0.5], 4, (160.0,), (160.0, 160.0, 160.0), (1.33, 0.001), [0.0, 30.0, 60.0, 90.0]),
        # a metal-like index, and n_r < 1
        "absorbing": _case([1.0, 3.0], 2, (0.5, 0.3), (0.015, 0.0, 0.015), [[2.0, 3.0], [0.3, 4.0]], [0.0, 10.0, 45.0, 90.0]),
        # x from 3.0e-3 to 3.0e-2, where the upward recurrence cancels; below that see DESIGN.md 4.5e
        "small-x": _case([10.0], 2, (0.02, 0.4), closed(10, 0.0048, 0.0047), (1.4, 0.01), [0.0, 45.0, 90.0]),
        # the range ends after 26 radii; from index 93 on the series of the same block's radii fail with code 2
        "fail-behind-cut": _case([0.5], 2, (0.5, 0.3), (0.1, 0.0, 0.1), (1.05, 0.0), [0.0, 90.0]),
        "closed-2": _case(even["wavel"], 2, even["dsize"], closed(2), even["m"], [0.0, 90.0]),
        "theta-0": _case(even["wavel"], 2, even["dsize"], even["rs"], even["m"], [0.0]),
        "theta-90": _case(even["wavel"], 2, even["dsize"], even["rs"], even["m"], [90.0]),
        "theta-33": _case(even["wavel"], 2, even["dsize"], even["rs"], even["m"], theta33),
        "theta-33-90": _case(even["wavel"], 2, even["dsize"], even["rs"], even["m"], np.append(theta33[:32], 90.0)),
        "waves-130": _case(w130, 2, even["dsize"], closed(12), np.stack([np.linspace(1.3, 1.6, 130), np.linspace(0.0, 0.05, 130)], axis=1),
                           [0.0, 30.0, 90.0]),
        # 300 radii, x up to 829: at the default block of 512 radii the workspace would take 1.7 GiB, so the block is halved
        "ws-halved": _case(w64, 2, (62.0, 0.05), closed(300, 60.0), np.stack([np.linspace(1.33, 1.5, 64), np.linspace(0.0, 0.01, 64)], axis=1),
                           [0.0, 30.0, 90.0]),
    }
    for name, step in OPEN_STEPS.items():
        cases[name] = _case([0.8], 2, (0.5, 0.3), (step, 0.0, step), (1.4, 0.01), [0.0, 90.0])
    return cases


EDGE_EXPECTED_RADII = {"perwave-m": [177, 208, 209], "nmx150": 50, "x2000-single": 1, "absorbing": [147, 146], "small-x": 10,
                       "fail-behind-cut": 26, "closed-2": 2, "theta-0": 10, "theta-90": 10, "theta-33": 10, "theta-33-90": 10,
                       "waves-130": 12, "ws-halved": 300, "open-64": 64, "open-65": 65, "open-128": 128, "open-129": 129}
EDGE_OPEN_CASES = ("perwave-m", "absorbing", "fail-behind-cut") + tuple(OPEN_STEPS)


def one_ulp_sensitivity(case):
    """how strongly a case amplifies a last-place difference in sin, cos, exp, log and pow: the larger of the deviations
    of makephase_np from itself with those results shifted by one ulp one way (cos, exp, log, pow up, sin down) and the other"""
    run = lambda fn: makephase_np(case["wavel"], case["iscat"], case["dsize"], case["rs"], case["refindx"], case["theta"],
                                  return_counts=True, fn=fn)
    base = run(NUMPY_FUNCS)
    g = dict(xscat=base[0], xext=base[1], phas=base[3])
    devs = []
    for direction in (1.0, -1.0):
        got = run(shifted_funcs(direction))
        assert np.array_equal(got[4], base[4]), (got[4], base[4])
        devs.append(deviations((got[0], got[1], got[3]), g))
    return tuple(max(a, b) for a, b in zip(*devs))


def load_golden(path):
    z = np.load(path)
    out = {}
    for key in z.files:
        name, field = key.split("__")
        out.setdefault(name, {})[field] = z[key]
    return out


def deviations(got, g):
    """(cross-sections, phase max-norm, phase pointwise): the three relative deviations of (xscat, xext, phas) from a golden"""
    xs, xe, ph = got
    cross = max(np.max(np.abs(xs - g["xscat"]) / g["xscat"]), np.max(np.abs(xe - g["xext"]) / g["xext"]))
    norm = np.max(np.max(np.abs(ph - g["phas"]), axis=1) / np.max(np.abs(g["phas"]), axis=1))
    point = np.max(np.abs(ph - g["phas"]) / np.abs(g["phas"]))
    return float(cross), float(norm), float(point)
