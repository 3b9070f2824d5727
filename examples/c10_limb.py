#!/usr/bin/env python
"""A limb sounder on the GPU from end to end: the thermal emission at a few tangent heights and its gradient with respect to a
temperature profile, from a synthetic k-table atmosphere -- what nemesisLfmg computes, with the limb paths that bracket each
tangent height mixed on the device before anything of the size of dSPECOUT (NWAVE, NPAR, LIMAX, NPATH) exists.  No reference
needed.

    python examples/c10_limb.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import archnemesis_dist_amd as pkg
from archnemesis_dist_amd import synthetic as syn, limb


def main():
    eng = pkg.AnsfmEngine(0)
    W, G, S, L, NPRO = 512, 10, 3, 40, 40
    PRESS, TEMP, K = syn.synth_ktable(W, G, 8, 6, S, seed=1)
    WAVE = 600.0 + 0.5 * np.arange(W)
    eng.upload_ktable(K, PRESS, TEMP, WAVE, syn.gauss_legendre_01(G)[1])
    atm = syn.synth_atmosphere(L, S, seed=2)
    lp, lt, am = atm["lay_press_pa"][0], atm["lay_temp"][0], atm["amount"][0]
    RADIUS = 7.0e7                                                   # m
    BASEH = np.linspace(0.0, 1.2e6, L + 1)[:-1]
    top = np.append(BASEH[1:], 2 * BASEH[-1] - BASEH[-2])
    TANHE = np.array([200.0, 450.0, 700.0, 950.0])                   # km: the geometries of the measurement
    # the two limb paths that bracket each tangent height, as calc_pathg_L lays them out: down from the top to the tangent layer
    # and up again, every entry emitting at its layer's temperature
    below = np.searchsorted(BASEH / 1.0e3, TANHE, side="right") - 1
    bottoms = np.stack([below, below + 1], axis=1).reshape(-1)
    P = bottoms.size
    LAYINC = np.zeros((2 * L, P), dtype=np.int32); SCALE = np.zeros((2 * L, P)); NLAYIN = np.zeros(P, dtype=np.int32)
    EMTEMP = np.zeros((2 * L, P))
    for p, b in enumerate(bottoms):
        lay = np.arange(b, L)
        r0 = RADIUS + BASEH[b]
        chord = np.sqrt((RADIUS + top[lay]) ** 2 - r0 ** 2) - np.sqrt(np.maximum((RADIUS + BASEH[lay]) ** 2 - r0 ** 2, 0.0))
        s = chord / (top[lay] - BASEH[lay])                          # slant length over layer thickness
        n = 2 * lay.size
        NLAYIN[p] = n
        LAYINC[:n, p] = np.concatenate([lay[::-1], lay]); SCALE[:n, p] = np.concatenate([s[::-1], s])
        EMTEMP[:n, p] = lt[LAYINC[:n, p]]
    tan = limb.tangent_heights_km(BASEH, NLAYIN, LAYINC)
    C = limb.tangent_mix(tan, TANHE)                                 # (NGEOM, NPATH): two entries a row
    Q = C.shape[0]
    NVMR, NDUST = S, 0
    NPAR = NVMR + 2 + NDUST
    MOD, SPEC, _ = eng.cirsradg_ck_limb(0, lp, lt, am, None, None, NVMR, NPAR, np.arange(S, dtype=np.int32), NLAYIN, LAYINC, SCALE, EMTEMP,
                                        C, gradients_on_device=True)
    scratch, ms_sens, ms_grad = eng.limb_last()
    # layers -> levels -> state vector on the device: one layer per level here, the state vector is the temperature profile
    eye = np.eye(L, NPRO)
    xmap = np.zeros((NPRO, NPAR, NPRO)); xmap[np.arange(NPRO), NVMR, np.arange(NPRO)] = 1.0
    eng.map2pro(None, W, NVMR, NDUST, NPRO, Q, np.array([L] * Q), np.tile(np.arange(L)[:, None], (1, Q)), eye, eye, eye, INCPAR=[NVMR],
                to_host=False)
    dmod = eng.map2xvec(None, W, NVMR, NDUST, NPRO, Q, NPRO, xmap)   # (W, Q, NPRO)
    for q in range(Q):
        i = int(np.argmax(MOD[:, q]))                               # the brightest wavenumber of this line of sight
        lev = int(np.argmax(np.abs(dmod[i, q])))
        print("tangent height %6.1f km (paths at %.1f / %.1f km): radiance %.3e .. %.3e W cm-2 sr-1 (cm-1)-1, brightest at %.1f cm-1; "
              "d R / d T(level) there largest at level %d (%.1f km): %.3e / K" % (TANHE[q], tan[2 * q], tan[2 * q + 1], MOD[:, q].min(),
                                                                                 MOD[:, q].max(), WAVE[i], lev, BASEH[lev] / 1.0e3,
                                                                                 dmod[i, q, lev]))
    print("k_limb_planck + k_limb_sens %.3f ms, k_limb_grad %.3f ms, %.2f MB of scratch beyond the gas stage, dMOD %.1f MB (dSPECOUT "
          "would be %.1f MB)" % (ms_sens, ms_grad, scratch / 1e6, 8e-6 * W * NPAR * L * Q, 8e-6 * W * NPAR * 2 * L * P))
    eng.close()


if __name__ == "__main__":
    main()
