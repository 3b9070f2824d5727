"""Primary-transit depth with gradients (nemesisPTfm, ForwardModel_0.py:1838-1995) restated in NumPy -- the written-down
contract of the kernels in csrc/ansfm_transit_kernels.hip.h and of AnsfmEngine.cirsradg_ck_transit.

Two forms of the same algebra:
  un-collapsed   the reference's: SPECOUT (W, P) and dSPECOUT (W, NPAR, LIMAX, P) of the transmission branch of CIRSrad, then
                 the trapezoid over tangent height (`area_from_paths`);
  collapsed      what the device does: the path matrix Sm, AREA and dAREA (W, NPAR, L) without any array over (LIMAX, P)
                 (`collapsed`).
"""
import numpy as np


def tangent_heights_km(BASEH, NLAYIN, LAYINC):
    """BASEH_TANHE (:1906-1908), km"""
    P = len(NLAYIN)
    return np.array([BASEH[LAYINC[int(NLAYIN[i] / 2), i]] / 1.0e3 for i in range(P)])


def path_weights(tanhe_km, RADIUS):
    """c_p: sum_i 0.5 (S_i + S_{i+1}) dH_i with S_i = (1 - T_i) 2 pi (h_i + RADIUS) (:1949-1954) collected by path"""
    P = len(tanhe_km)
    c = np.zeros(P)
    for i in range(P - 1):
        dH = (tanhe_km[i + 1] - tanhe_km[i]) * 1.0e3
        c[i] += 0.5 * dH * 2. * np.pi * (tanhe_km[i] * 1.0e3 + RADIUS)
        c[i + 1] += 0.5 * dH * 2. * np.pi * (tanhe_km[i + 1] * 1.0e3 + RADIUS)
    return c


def path_matrix(L, NLAYIN, LAYINC, SCALE):
    """Sm[l][p] = sum of SCALE[j, p] over j < NLAYIN[p] with LAYINC[j, p] = l; padding entries are not read"""
    P = len(NLAYIN)
    Sm = np.zeros((L, P))
    for p in range(P):
        for j in range(int(NLAYIN[p])):
            Sm[LAYINC[j, p], p] += SCALE[j, p]
    return Sm


def dtautot(dk, igas_map, NVMR, NPAR, dtaucon=None, dtau_every_gas=None, gases=None, temperature=True):
    """dTAUTOT (W, G, NPAR, L) from the gradient merge's dk (W, G, L, S + 1) as :3868-3872, :3993 assemble it.  gases: the
    selection of set_gradient_gases (None = all)."""
    W, G, L, S1 = dk.shape
    out = np.zeros((W, G, NPAR, L))
    for i in range(S1 - 1):
        if gases is None or i in gases:
            out[:, :, igas_map[i], :] = dk[:, :, :, i] * 1.0e-4
    out[:, :, NVMR, :] = dk[:, :, :, S1 - 1] if temperature else 0.0
    if dtaucon is not None:
        out += np.asarray(dtaucon)[:, None, :, :]
    if dtau_every_gas is not None:
        out[:, :, :NVMR, :] += np.asarray(dtau_every_gas)[:, None, None, :]
    return out


def collapsed(tautot, delg, Sm, c, dtau=None):
    """tautot (W, G, L), dtau (W, G, NPAR, L) -> AREA (W,), TRANS (W, P), dAREA (W, NPAR, L) (None without dtau)"""
    e = np.exp(-np.einsum("wgl,lp->wgp", tautot, Sm))                  # exp(-tau_path)
    TRANS = np.einsum("wgp,g->wp", e, delg)
    AREA = (1.0 - TRANS) @ c
    if dtau is None:
        return AREA, TRANS, None
    A = np.einsum("wgp,p,lp->wgl", e, c, Sm)
    dAREA = np.nan_to_num(np.einsum("g,wgl,wgkl->wkl", delg, A, dtau))
    return AREA, TRANS, dAREA


def uncollapsed(tautot, delg, NLAYIN, LAYINC, SCALE, dtau):
    """The transmission branch of CIRSrad(return_grad=True) (:4006-4012, :4110-4131, :4504-4507): SPECOUT (W, P),
    dSPECOUT (W, NPAR, LIMAX, P)"""
    LIMAX, P = LAYINC.shape
    inside = np.arange(LIMAX)[:, None] < np.asarray(NLAYIN)[None, :]
    sc = np.where(inside, SCALE, 0.0)
    li = np.where(inside, LAYINC, 0)
    sg = np.exp(-np.sum(tautot[:, :, li] * sc, axis=2))               # (W, G, P)
    dlay = dtau[:, :, :, li] * sc                                      # (W, G, NPAR, LIMAX, P)
    dspec = np.nan_to_num(np.tensordot(-sg[:, :, None, None, :] * dlay, delg, axes=([1], [0])))
    return np.tensordot(sg, delg, axes=([1], [0])), dspec


def area_from_paths(SPECOUT, dSPECOUT, c, NLAYIN, LAYINC, L):
    """The trapezoid applied to the un-collapsed arrays: AREA (W,) and dAREA (W, NPAR, L), every (entry, path) of dSPECOUT
    handed to its layer with the weight -c_p"""
    W, NPAR, LIMAX, P = dSPECOUT.shape
    AREA = (1.0 - SPECOUT) @ c
    dAREA = np.zeros((W, NPAR, L))
    for p in range(P):
        for j in range(int(NLAYIN[p])):
            dAREA[:, :, LAYINC[j, p]] -= c[p] * dSPECOUT[:, :, j, p]
    return AREA, dAREA


def depth(AREA, RADIUS, tanhe0_km, RSTAR_KM):
    """SPECMOD (:1941-1944, :1963): the transit depth in per cent; the factor of dSPECMOD (:1966) is 100 / area_star"""
    area_star = np.pi * ((RSTAR_KM * 1.0e3) ** 2)
    area_planet_disk = np.pi * ((RADIUS + tanhe0_km * 1.0e3) ** 2)
    return (AREA + area_planet_disk) / area_star * 100., 100. / area_star


def limb_paths(L, rng):
    """Paths shaped as calc_path_PT makes them: path p runs from the top layer down to layer p and up again"""
    P = L - 1
    LAYINC = np.zeros((2 * L, P), dtype=np.int32)
    NLAYIN = np.zeros(P, dtype=np.int32)
    for p in range(P):
        n = 2 * (L - p)
        LAYINC[:n, p] = np.concatenate([np.arange(L - 1, p - 1, -1), np.arange(p, L)])
        NLAYIN[p] = n
    SCALE = np.where(np.arange(2 * L)[:, None] < NLAYIN[None, :], rng.uniform(1.0, 30.0, (2 * L, P)), 0.0)
    return NLAYIN, LAYINC, SCALE
