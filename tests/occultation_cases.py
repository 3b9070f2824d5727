"""Solar occultation with gradients (nemesisSOfmg, ForwardModel_0.py:983-1249) restated in NumPy -- the written-down contract of
the kernels in csrc/ansfm_occultation_kernels.hip.h, of AnsfmEngine.cirsradg_ck_occultation and of occultation.tangent_mix.

Two forms of the same algebra:
  un-collapsed   the reference's: SPECOUT (W, P) and dSPECOUT (W, NPAR, LIMAX, P) of the transmission branch of CIRSrad, then
                 the mix of the paths to the geometries (`mod_from_paths`);
  collapsed      what the device does: the path matrix Sm and the mixing matrix C, MOD (W, Q) and dMOD (W, NPAR, L, Q) without
                 any array over (LIMAX, P) (`collapsed`).
"""
import numpy as np

from transit_cases import path_matrix, dtautot, limb_paths, uncollapsed, tangent_heights_km  # noqa: F401


def tangent_mix(BASEH_TANHE_km, TANHE):
    """C (NGEOM, NPATH): the interpolation of :1211-1232 written as the matrix that SPECMOD = SPECOUT @ C.T applies.  The loop is
    the reference's, index for index: a Python index of -1 is the last path."""
    B = np.asarray(BASEH_TANHE_km, dtype=np.float64)
    T = np.asarray(TANHE, dtype=np.float64).reshape(len(TANHE), -1)[:, 0]
    NPATH = B.size
    C = np.zeros((T.size, NPATH))
    eye = np.eye(NPATH)
    for i in range(T.size):
        ibase = np.argmin(np.abs(B - T[i]))
        base0 = B[ibase]
        if base0 <= T[i]:
            ibasel = ibase
            ibaseh = ibase + 1
        else:
            ibasel = ibase - 1
            ibaseh = ibase
        if ibaseh > NPATH - 1:
            C[i] = eye[ibasel]
        else:
            fhl = (T[i] - B[ibasel]) / (B[ibaseh] - B[ibasel])
            fhh = (B[ibaseh] - T[i]) / (B[ibaseh] - B[ibasel])
            C[i] = eye[ibasel] * (1. - fhl) + eye[ibaseh] * (1. - fhh)
    return C


def collapsed(tautot, delg, Sm, C, dtau=None, xfac=None):
    """tautot (W, G, L), dtau (W, G, NPAR, L), C (Q, P) -> MOD (W, Q), TRANS (W, P), dMOD (W, NPAR, L, Q) (None without dtau)"""
    xf = np.ones(tautot.shape[0]) if xfac is None else np.asarray(xfac, dtype=np.float64)
    e = np.exp(-np.einsum("wgl,lp->wgp", tautot, Sm))                  # exp(-tau_path)
    TRANS = np.einsum("wgp,g->wp", e, delg)
    MOD = xf[:, None] * (TRANS @ C.T)
    if dtau is None:
        return MOD, TRANS, None
    B = np.einsum("qp,lp,wgp->wglq", C, Sm, e)
    dMOD = np.nan_to_num(-xf[:, None, None, None] * np.einsum("g,wglq,wgkl->wklq", delg, B, dtau))
    return MOD, TRANS, dMOD


def mod_from_paths(SPECOUT, dSPECOUT, C, NLAYIN, LAYINC, L):
    """The mix applied to the un-collapsed arrays: MOD (W, Q) and dMOD (W, NPAR, L, Q), every (entry, path) of dSPECOUT handed
    to its layer with the weight C[q, p].  SPECOUT / dSPECOUT carry xfac already, as CIRSrad returns them."""
    W, NPAR, LIMAX, P = dSPECOUT.shape
    Q = C.shape[0]
    MOD = SPECOUT @ C.T
    dMOD = np.zeros((W, NPAR, L, Q))
    for p in range(P):
        for j in range(int(NLAYIN[p])):
            dMOD[:, :, LAYINC[j, p], :] += dSPECOUT[:, :, j, p][:, :, None] * C[None, None, :, p]
    return MOD, dMOD


def occultation_paths(L, Q, rng):
    """Pairs of limb paths as calc_pathg_SO makes them: for each of Q tangent heights the two paths whose lowest layers bracket
    it (layers b and b + 1), each from the top layer down to its lowest layer and up again.  -> NLAYIN (2 Q,), LAYINC / SCALE
    (2 L, 2 Q), bottoms (2 Q,)"""
    NL, LAYINC_all, _ = limb_paths(L, rng)
    lows = np.sort(rng.choice(np.arange(0, L - 2), size=Q, replace=False)) if Q <= L - 2 else np.arange(Q) % (L - 2)
    bottoms = np.stack([lows, lows + 1], axis=1).reshape(-1)
    NLAYIN = np.ascontiguousarray(NL[bottoms])
    LAYINC = np.ascontiguousarray(LAYINC_all[:, bottoms])
    SCALE = np.where(np.arange(2 * L)[:, None] < NLAYIN[None, :], rng.uniform(1.0, 30.0, (2 * L, 2 * Q)), 0.0)
    return NLAYIN, LAYINC, SCALE, bottoms
