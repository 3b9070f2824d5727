"""Limb thermal emission with gradients (nemesisLfmg, ForwardModel_0.py:1372-1521) restated in NumPy -- the written-down contract
of the kernels in csrc/ansfm_limb_kernels.hip.h, of AnsfmEngine.cirsradg_ck_limb and of limb.tangent_mix.

Two forms of the same algebra:
  un-collapsed   the reference's: SPECOUT (W, P) and dSPECOUT (W, NPAR, LIMAX, P) of the thermal-emission branch of CIRSrad on limb
                 paths (`uncollapsed`), then the mix of the paths to the geometries (`mod_from_paths`);
  collapsed      what the device does: MOD (W, Q) and dMOD (W, NPAR, L, Q) through E (W, G, L, Q) and Z (W, L, Q) without any
                 array over (LIMAX, P) (`collapsed`).
"""
import numpy as np

from occultation_cases import tangent_mix, mod_from_paths, occultation_paths  # noqa: F401
from transit_cases import dtautot, limb_paths, tangent_heights_km  # noqa: F401


def planckg(ispace, wave, temp):
    """bb, dBdT (:6263-6281)"""
    c1 = 1.1911e-12
    c2 = 1.439
    if ispace == 0:
        y = wave
        a = c1 * (y ** 3.)
        ap = c1 * c2 * (y ** 4.) / temp ** 2.
    else:
        y = 1.0e4 / wave
        a = c1 * (y ** 5.) / 1.0e4
        ap = c1 * c2 * (y ** 6.) / 1.0e4 / temp ** 2.
    tmp = c2 * y / temp
    b = np.exp(tmp) - 1
    return a / b, np.exp(tmp) * ap / b ** 2.


def _path(tautot, wave, ispace, n, li, sc, th):
    """T_{j-1} - T_j (W, G, n), T_j (W, G, n), B and dB/dT (W, n) along one path: the product form of :6446-6452"""
    T = np.cumprod(np.exp(-tautot[:, :, li] * sc[None, None, :]), axis=2)
    Tprev = np.concatenate([np.ones_like(T[:, :, :1]), T[:, :, :-1]], axis=2)
    B = np.empty((wave.size, n)); dB = np.empty((wave.size, n))
    for j in range(n):
        B[:, j], dB[:, j] = planckg(ispace, wave, th[j])
    return Tprev - T, T, B, dB


def is_limb_path(lay_press, NLAYIN, LAYINC, p):
    """the test of :6479-6483: the lower boundary contributes when the last layer lies deeper than the middle one"""
    n = int(NLAYIN[p])
    return not lay_press[LAYINC[n - 1, p]] > lay_press[LAYINC[int(n / 2) - 1, p]]


def uncollapsed(tautot, delg, NLAYIN, LAYINC, SCALE, EMTEMP, ispace, wave, NVMR, dtau=None, xfac=None):
    """The thermal-emission branch of CIRSrad(return_grad=True) on limb paths (:4006-4012, :6444-6476, :4247, :4504-4507):
    SPECOUT (W, P) and dSPECOUT (W, NPAR, LIMAX, P), both times xfac; the tail sum of d spec / d tau_j summed directly"""
    W, G, L = tautot.shape
    LIMAX, P = LAYINC.shape
    xf = np.ones(W) if xfac is None else np.asarray(xfac, dtype=np.float64)
    SPECOUT = np.zeros((W, P))
    dSPECOUT = None if dtau is None else np.zeros((W, dtau.shape[2], LIMAX, P))
    for p in range(P):
        n = int(NLAYIN[p])
        if n == 0:
            continue
        li, sc = LAYINC[:n, p], SCALE[:n, p]
        d, T, B, dB = _path(tautot, wave, ispace, n, li, sc, EMTEMP[:n, p])
        e = d * B[:, None, :]
        SPECOUT[:, p] = np.einsum("wgj,g->w", e, delg) * xf
        if dtau is None:
            continue
        tail = np.cumsum(e[:, :, ::-1], axis=2)[:, :, ::-1] - e                    # sum_{m > j}
        A = T * B[:, None, :] - tail
        ds = dtau[:, :, :, li] * (sc[None, None, :] * A)[:, :, None, :]           # (W, G, NPAR, n)
        ds[:, :, NVMR, :] += d * dB[:, None, :]
        dSPECOUT[:, :, :n, p] = np.nan_to_num(np.einsum("wgkj,g->wkj", ds, delg) * xf[:, None, None])
    return SPECOUT, dSPECOUT


def collapsed(tautot, delg, NLAYIN, LAYINC, SCALE, EMTEMP, C, ispace, wave, NVMR, dtau=None, xfac=None):
    """C (Q, P) -> MOD (W, Q), SPEC (W, P) before xfac, dMOD (W, NPAR, L, Q) (None without dtau); the tail sum formed as
    spec - prefix, as the device forms it"""
    W, G, L = tautot.shape
    Q, P = C.shape
    xf = np.ones(W) if xfac is None else np.asarray(xfac, dtype=np.float64)
    SPEC = np.zeros((W, P))
    E = np.zeros((W, G, L, Q)); Z = np.zeros((W, L, Q))
    for p in range(P):
        n = int(NLAYIN[p])
        if n == 0:
            continue
        li, sc = LAYINC[:n, p], SCALE[:n, p]
        d, T, B, dB = _path(tautot, wave, ispace, n, li, sc, EMTEMP[:n, p])
        e = d * B[:, None, :]
        spec = e.sum(axis=2)
        SPEC[:, p] = spec @ delg
        if dtau is None or not np.any(C[:, p] != 0):
            continue
        A = (T * B[:, None, :] - (spec[:, :, None] - np.cumsum(e, axis=2))) * sc[None, None, :]
        z = np.einsum("wgj,g->wj", d, delg) * dB
        for j in range(n):
            E[:, :, li[j], :] += A[:, :, j, None] * C[None, None, :, p]
            Z[:, li[j], :] += z[:, j, None] * C[None, :, p]
    MOD = xf[:, None] * (SPEC @ C.T)
    if dtau is None:
        return MOD, SPEC, None
    dMOD = np.einsum("g,wglq,wgkl->wklq", delg, E, dtau)
    dMOD[:, NVMR] += Z
    return MOD, SPEC, np.nan_to_num(xf[:, None, None, None] * dMOD)


def limb_pairs(L, Q, rng):
    """occultation_paths (the bracketing pairs of calc_pathg_L) with an EMTEMP of its own for every entry: the two legs of a path
    differ in SCALE and in EMTEMP.  -> NLAYIN, LAYINC, SCALE, EMTEMP, bottoms"""
    NLAYIN, LAYINC, SCALE, bottoms = occultation_paths(L, Q, rng)
    EMTEMP = np.where(np.arange(2 * L)[:, None] < NLAYIN[None, :], rng.uniform(120.0, 260.0, SCALE.shape), 0.0)
    return NLAYIN, LAYINC, SCALE, EMTEMP, bottoms


def cancellation_terms(tautot, delg, NLAYIN, LAYINC, SCALE, EMTEMP, C, ispace, wave, NVMR, dtau, xfac=None):
    """What the rounding of d_j = T_{j-1} - T_j can cost dMOD, element by element: (W, NPAR, L, Q), non-negative, in units of the
    relative rounding of one operation.  T_j = T_{j-1} exp(-tau_j) carries the rounding of exp and of the product, and the
    subtraction one more, so d_j is off by a few 2^-53 T_{j-1} whatever tau_j is -- a relative error of 2^-53 / tau_j, which a thin
    layer (tau ~ 1e-9) turns into 1e-7.  d enters A_j through its tail sum and through T_j itself, and Z directly:
        |delta A_j| <= u (T_j B_j + sum_{m > j} T_{m-1} B_m),        |delta Z_j| <= u T_{j-1} dB/dT_j,
    and everything after that is linear; this returns the right-hand sides carried through the mix and the contraction with
    absolute values throughout."""
    W, G, L = tautot.shape
    Q, P = C.shape
    xf = np.ones(W) if xfac is None else np.abs(np.asarray(xfac, dtype=np.float64))
    E = np.zeros((W, G, L, Q)); Z = np.zeros((W, L, Q))
    Ca = np.abs(C)
    for p in range(P):
        n = int(NLAYIN[p])
        if n == 0 or not np.any(Ca[:, p] != 0):
            continue
        li, sc = LAYINC[:n, p], SCALE[:n, p]
        d, T, B, dB = _path(tautot, wave, ispace, n, li, sc, EMTEMP[:n, p])
        Tprev = d + T
        e = Tprev * B[:, None, :]
        tail = np.cumsum(e[:, :, ::-1], axis=2)[:, :, ::-1] - e
        A = (T * B[:, None, :] + tail) * sc[None, None, :]
        z = np.einsum("wgj,g->wj", Tprev, delg) * np.abs(dB)
        for j in range(n):
            E[:, :, li[j], :] += A[:, :, j, None] * Ca[None, None, :, p]
            Z[:, li[j], :] += z[:, j, None] * Ca[None, :, p]
    out = np.einsum("g,wglq,wgkl->wklq", delg, E, np.abs(dtau))
    out[:, NVMR] += Z
    return xf[:, None, None, None] * out


def golden_cancellation_by_column(z, oracle):
    """cancellation_terms on a golden fixture (limb_c1.npz) carried to the state vector with the absolute values of the maps, over
    the largest element of the reference's dSPECMOD column: (NX,), what one unit of relative rounding in every d_j can cost a
    column relative to its largest element (0 for the columns the reference leaves zero)"""
    L = z["LAY_PRESS"].size
    NVMR, NDUST, NPRO = int(z["NVMR"]), int(z["NDUST"]), int(z["NPRO"])
    C = tangent_mix(tangent_heights_km(z["BASEH"], z["NLAYIN"], z["LAYINC"]), z["TANHE"])
    Q = C.shape[0]
    ct = cancellation_terms(z["TAUTOT"], np.asarray(z["DELG"], dtype=np.float64), z["NLAYIN"], z["LAYINC"], z["SCALE"], z["EMTEMP"], C,
                            int(z["ISPACE"]), z["WAVE"], NVMR, z["dTAUTOT"], z["XFAC"])
    W, NX = ct.shape[0], z["xmap"].shape[0]
    pro = oracle.map2pro(ct, W, NVMR, NDUST, NPRO, Q, np.array([L] * Q), np.tile(np.arange(L)[:, None], (1, Q)), np.abs(z["DTE"]),
                         np.abs(z["DAM"]), np.abs(z["DCO"]), INCPAR=list(z["incpar"]))
    d = oracle.map2xvec(pro, W, NVMR, NDUST, NPRO, Q, NX, np.abs(z["xmap"]))
    scale = np.abs(z["dSPECMOD"]).max(axis=(0, 1))
    return np.where(scale > 0, d.max(axis=(0, 1)) / np.where(scale > 0, scale, 1.0), 0.0)
