"""Disc-averaged thermal emission with gradients (nemesisdiscfmg, ForwardModel_0.py:1719-1834) restated in NumPy -- the
written-down contract of the kernels in csrc/ansfm_disc_kernels.hip.h, of AnsfmEngine.cirsradg_ck_disc and of disc.average_mix.

The averaging points of a geometry are P paths through ONE layer sequence (LAYINC (N,), EMTEMP (N,)) that differ in SCALE (N, P)
only; the sequence may end at the lower boundary (:6479-6498).  Two forms of the same algebra:
  un-collapsed   the reference's: SPECOUT (W, P), dSPECOUT (W, NPAR, N, P) and dTSURF (W, P) of the thermal-emission branch of
                 CIRSrad path by path (`uncollapsed`), then the weighted sum of the points (`mod_from_points`);
  collapsed      what the device does: MOD (W, Q), dTSMOD (W, Q) and dMOD (W, NPAR, L, Q) through E (W, G, L, Q) and Z (W, L, Q)
                 without any array over (N, P) (`collapsed`).
"""
import numpy as np

from limb_cases import planckg  # noqa: F401
from transit_cases import dtautot  # noqa: F401


def is_ground(lay_press, LAYINC):
    """the test of :6479-6483: the lower boundary contributes when the last layer lies deeper than the middle one (the index
    int(N / 2) - 1 = -1 of a one-entry sequence wraps, as in Python)"""
    n = len(LAYINC)
    return bool(lay_press[LAYINC[n - 1]] > lay_press[LAYINC[int(n / 2) - 1]])


def ground_radiance(ispace, wave, EMTEMP, TSURF, EMISSIVITY):
    """R, dR (W,) of :6485-6491"""
    if TSURF <= 0.0:
        return planckg(ispace, wave, EMTEMP[-1])
    b, db = planckg(ispace, wave, TSURF)
    return b * EMISSIVITY, db * EMISSIVITY


def _paths(tautot, wave, ispace, LAYINC, SCALE, EMTEMP):
    """T_{j-1} - T_j and T_j (W, G, N, P), B and dB/dT (W, N): the product form of :6446-6452 for every path at once"""
    N = len(LAYINC)
    T = np.cumprod(np.exp(-tautot[:, :, LAYINC, None] * SCALE[None, None, :, :]), axis=2)
    Tprev = np.concatenate([np.ones_like(T[:, :, :1]), T[:, :, :-1]], axis=2)
    B = np.empty((wave.size, N)); dB = np.empty((wave.size, N))
    for j in range(N):
        B[:, j], dB[:, j] = planckg(ispace, wave, EMTEMP[j])
    return Tprev - T, T, B, dB


def uncollapsed(tautot, delg, lay_press, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, ispace, wave, NVMR, dtau=None, xfac=None):
    """The thermal-emission branch of CIRSrad(return_grad=True) on each path (:4006-4012, :6444-6502, :4244-4247, :4504-4507):
    SPECOUT (W, P), dSPECOUT (W, NPAR, N, P) and dTSURF (W, P), all times xfac; the tail sum of d spec / d tau_j summed directly"""
    W, G, L = tautot.shape
    N, P = SCALE.shape
    xf = np.ones(W) if xfac is None else np.asarray(xfac, dtype=np.float64)
    d, T, B, dB = _paths(tautot, wave, ispace, LAYINC, SCALE, EMTEMP)
    e = d * B[:, None, :, None]
    spec = e.sum(axis=2)                                                        # (W, G, P)
    ground = is_ground(lay_press, LAYINC)
    dts = np.zeros((W, G, P))
    if ground:
        R, dR = ground_radiance(ispace, wave, EMTEMP, TSURF, EMISSIVITY)
        spec = spec + T[:, :, -1, :] * R[:, None, None]
        dts = T[:, :, -1, :] * dR[:, None, None]
    SPECOUT = np.einsum("wgp,g->wp", spec, delg) * xf[:, None]
    dTSURF = np.einsum("wgp,g->wp", dts, delg) * xf[:, None]
    if dtau is None:
        return SPECOUT, None, dTSURF
    tail = np.cumsum(e[:, :, ::-1], axis=2)[:, :, ::-1] - e                      # sum_{m > j}
    A = T * B[:, None, :, None] - tail
    if ground:
        A = A - (T[:, :, -1, :] * R[:, None, None])[:, :, None, :]              # :6498
    ds = dtau[:, :, :, LAYINC, None] * (SCALE[None, None, :, :] * A)[:, :, None, :, :]          # (W, G, NPAR, N, P)
    ds[:, :, NVMR] += d * dB[:, None, :, None]
    dSPECOUT = np.nan_to_num(np.einsum("wgkjp,g->wkjp", ds, delg) * xf[:, None, None, None])
    return SPECOUT, dSPECOUT, dTSURF


def mod_from_points(SPECOUT, dSPECOUT, dTSURF, C, LAYINC, L):
    """The weighted sum of :1789-1794 on the un-collapsed arrays: MOD (W, Q), dTSMOD (W, Q), dMOD (W, NPAR, L, Q)"""
    W, NPAR, N, P = dSPECOUT.shape
    Q = C.shape[0]
    dMOD = np.zeros((W, NPAR, L, Q))
    mixed = np.einsum("wkjp,qp->wkjq", dSPECOUT, C)
    for j in range(N):
        dMOD[:, :, LAYINC[j], :] += mixed[:, :, j, :]
    return SPECOUT @ C.T, dTSURF @ C.T, dMOD


def collapsed(tautot, delg, lay_press, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, C, ispace, wave, NVMR, dtau=None, xfac=None):
    """C (Q, P) -> MOD (W, Q), SPEC (W, P) before xfac, dTSMOD (W, Q), dMOD (W, NPAR, L, Q) (None without dtau); the tail sum
    formed as spec_atm - prefix and the ground's term subtracted explicitly, as the device forms them"""
    W, G, L = tautot.shape
    N, P = SCALE.shape
    Q = C.shape[0]
    xf = np.ones(W) if xfac is None else np.asarray(xfac, dtype=np.float64)
    d, T, B, dB = _paths(tautot, wave, ispace, LAYINC, SCALE, EMTEMP)
    e = d * B[:, None, :, None]
    atm = e.sum(axis=2)                                                         # (W, G, P)
    ground = is_ground(lay_press, LAYINC)
    gt = np.zeros((W, G, P)); dts = np.zeros((W, G, P))
    if ground:
        R, dR = ground_radiance(ispace, wave, EMTEMP, TSURF, EMISSIVITY)
        gt = T[:, :, -1, :] * R[:, None, None]
        dts = T[:, :, -1, :] * dR[:, None, None]
    SPEC = np.einsum("wgp,g->wp", atm + gt, delg)
    MOD = xf[:, None] * (SPEC @ C.T)
    dTSMOD = xf[:, None] * (np.einsum("wgp,g->wp", dts, delg) @ C.T)
    if dtau is None:
        return MOD, SPEC, dTSMOD, None
    A = (T * B[:, None, :, None] - (atm[:, :, None, :] - np.cumsum(e, axis=2)) - gt[:, :, None, :]) * SCALE[None, None, :, :]
    Ej = np.einsum("wgjp,qp->wgjq", A, C)
    Zj = np.einsum("wgjp,g,qp->wjq", d, delg, C) * dB[:, :, None]
    E = np.zeros((W, G, L, Q)); Z = np.zeros((W, L, Q))
    for j in range(N):
        E[:, :, LAYINC[j], :] += Ej[:, :, j, :]
        Z[:, LAYINC[j], :] += Zj[:, j, :]
    dMOD = np.einsum("g,wglq,wgkl->wklq", delg, E, dtau)
    dMOD[:, NVMR] += Z
    return MOD, SPEC, dTSMOD, np.nan_to_num(xf[:, None, None, None] * dMOD)


def cancellation_terms(tautot, delg, lay_press, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, C, ispace, wave, NVMR, dtau, xfac=None):
    """limb_cases.cancellation_terms for the disc's paths, with the surface terms: what the rounding of d_j = T_{j-1} - T_j and of
    T_end can cost dMOD, element by element (W, NPAR, L, Q), non-negative, in units of the relative rounding of one operation.
        |delta A_j| <= u (T_j B_j + sum_{m > j} T_{m-1} B_m + [ground] N T_end |R|),        |delta Z_j| <= u T_{j-1} dB/dT_j:
    T_end is a product of N factors exp(-tau_j), each with the rounding of exp and of the product, so its relative error is at
    most 2 N u, entered here as N units against the 4 x 2^-53 the golden test multiplies by (twice what it needs).  The second
    return value is the same for dTSMOD (W, Q): N T_end |dR| through the mix."""
    W, G, L = tautot.shape
    N, P = SCALE.shape
    xf = np.ones(W) if xfac is None else np.abs(np.asarray(xfac, dtype=np.float64))
    Ca = np.abs(C)
    d, T, B, dB = _paths(tautot, wave, ispace, LAYINC, SCALE, EMTEMP)
    Tprev = d + T
    e = Tprev * B[:, None, :, None]
    tail = np.cumsum(e[:, :, ::-1], axis=2)[:, :, ::-1] - e
    A = T * B[:, None, :, None] + tail
    dts = np.zeros((W, G, P))
    if is_ground(lay_press, LAYINC):
        R, dR = ground_radiance(ispace, wave, EMTEMP, TSURF, EMISSIVITY)
        A = A + (N * T[:, :, -1, :] * np.abs(R)[:, None, None])[:, :, None, :]
        dts = N * T[:, :, -1, :] * np.abs(dR)[:, None, None]
    A = A * SCALE[None, None, :, :]
    Ej = np.einsum("wgjp,qp->wgjq", A, Ca)
    Zj = np.einsum("wgjp,g,qp->wjq", Tprev, delg, Ca) * np.abs(dB)[:, :, None]
    E = np.zeros((W, G, L, C.shape[0])); Z = np.zeros((W, L, C.shape[0]))
    for j in range(N):
        E[:, :, LAYINC[j], :] += Ej[:, :, j, :]
        Z[:, LAYINC[j], :] += Zj[:, j, :]
    out = np.einsum("g,wglq,wgkl->wklq", delg, E, np.abs(dtau))
    out[:, NVMR] += Z
    return xf[:, None, None, None] * out, xf[:, None] * (np.einsum("wgp,g->wp", dts, delg) @ Ca.T)


def golden_inputs(z, case=""):
    """(args of collapsed / cancellation_terms up to C, keyword part) of a capture in disc_c1.npz; case "" or "S_" (TSURF > 0)"""
    g = lambda k: z[case + k] if case + k in z.files else z[k]
    C = np.asarray(g("WGEOM"), dtype=np.float64).reshape(1, -1)
    emis = g("EMISSIVITY") if float(g("TSURF")) > 0 else None
    return (g("TAUTOT"), np.asarray(z["DELG"], dtype=np.float64), z["LAY_PRESS"], z["LAYINC"], g("SCALE"), z["EMTEMP"], float(g("TSURF")),
            emis, C, int(z["ISPACE"]), z["WAVE"], int(z["NVMR"])), dict(dtau=g("dTAUTOT"), xfac=z["XFAC"])


def golden_cancellation_by_column(z, oracle, case=""):
    """cancellation_terms on a capture of disc_c1.npz carried to the state vector with the absolute values of the maps, over the
    largest element of the reference's dSPEC column: (NX,), what one unit of relative rounding can cost a column relative to its
    largest element (0 for the columns the reference leaves zero); and the same for the dTSURF column, a scalar"""
    g = lambda k: z[case + k] if case + k in z.files else z[k]
    L = z["LAY_PRESS"].size
    NVMR, NDUST, NPRO = int(z["NVMR"]), int(z["NDUST"]), int(z["NPRO"])
    args, kw = golden_inputs(z, case)
    ct, cts = cancellation_terms(*args, kw["dtau"], kw["xfac"])
    W, NX = ct.shape[0], z["xmap"].shape[0]
    pro = oracle.map2pro(ct, W, NVMR, NDUST, NPRO, 1, np.array([L]), np.arange(L)[:, None], np.abs(z["DTE"]), np.abs(z["DAM"]),
                         np.abs(z["DCO"]), INCPAR=list(z["incpar"]))
    dcol = oracle.map2xvec(pro, W, NVMR, NDUST, NPRO, 1, NX, np.abs(z["xmap"]))[:, 0, :]
    scale = np.abs(g("dSPEC")).max(axis=0)
    ts = np.abs(g("dTSURF") @ np.asarray(g("WGEOM"), dtype=np.float64)).max()
    return np.where(scale > 0, dcol.max(axis=0) / np.where(scale > 0, scale, 1.0), 0.0), (cts.max() / ts if ts > 0 else 0.0)
