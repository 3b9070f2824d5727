#!/usr/bin/env python
"""A primary transit on the GPU from end to end: the transit depth and its gradient with respect to a temperature profile, from
a synthetic k-table atmosphere -- what nemesisPTfm(gradients=True) computes, with the annuli summed on the device before
anything of the size of dSPECOUT (NWAVE, NPAR, 2 NLAY, NLAY - 1) exists.  No reference needed.

    python examples/c8_transit.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import archnemesis_dist_amd as pkg
from archnemesis_dist_amd import synthetic as syn, transit


def main():
    eng = pkg.AnsfmEngine(0)
    W, G, S, L, NPRO = 512, 10, 3, 40, 40
    PRESS, TEMP, K = syn.synth_ktable(W, G, 8, 6, S, seed=1)
    WAVE = 1000.0 + 0.5 * np.arange(W)
    eng.upload_ktable(K, PRESS, TEMP, WAVE, syn.gauss_legendre_01(G)[1])
    atm = syn.synth_atmosphere(L, S, seed=2)
    lp, lt, am = atm["lay_press_pa"][0], atm["lay_temp"][0], atm["amount"][0]
    # one limb path per layer, as calc_path_PT lays them out: down from the top to the tangent layer and up again
    RADIUS, RSTAR_KM = 7.0e7, 7.0e5                                  # m, km
    BASEH = np.linspace(0.0, 1.2e6, L + 1)[:-1]
    P = L - 1
    LAYINC = np.zeros((2 * L, P), dtype=np.int32); SCALE = np.zeros((2 * L, P)); NLAYIN = np.zeros(P, dtype=np.int32)
    top = np.append(BASEH[1:], 2 * BASEH[-1] - BASEH[-2])
    for p in range(P):
        lay = np.arange(p, L)
        r0 = RADIUS + BASEH[p]
        chord = np.sqrt((RADIUS + top[lay]) ** 2 - r0 ** 2) - np.sqrt(np.maximum((RADIUS + BASEH[lay]) ** 2 - r0 ** 2, 0.0))
        s = chord / (top[lay] - BASEH[lay])                          # slant length over layer thickness
        n = 2 * lay.size
        NLAYIN[p] = n
        LAYINC[:n, p] = np.concatenate([lay[::-1], lay]); SCALE[:n, p] = np.concatenate([s[::-1], s])
    tan = transit.tangent_heights_km(BASEH, NLAYIN, LAYINC)
    c = transit.path_weights(tan, RADIUS)
    NVMR, NDUST = S, 0
    NPAR = NVMR + 2 + NDUST
    AREA, TRANS, _ = eng.cirsradg_ck_transit(lp, lt, am, None, None, NVMR, NPAR, np.arange(S, dtype=np.int32), NLAYIN, LAYINC, SCALE,
                                             c, gradients_on_device=True)
    scratch, ms_sens, ms_grad = eng.transit_last()
    area_star = np.pi * (RSTAR_KM * 1.0e3) ** 2
    depth = (AREA + np.pi * (RADIUS + tan[0] * 1.0e3) ** 2) / area_star * 100.
    # layers -> levels -> state vector on the device: one layer per level here, the state vector is the temperature profile
    eye = np.eye(L, NPRO)
    xmap = np.zeros((NPRO, NPAR, NPRO)); xmap[np.arange(NPRO), NVMR, np.arange(NPRO)] = 1.0
    eng.map2pro(None, W, NVMR, NDUST, NPRO, 1, np.array([L]), np.arange(L), eye, eye, eye, INCPAR=[NVMR], to_host=False)
    ddepth = eng.map2xvec(None, W, NVMR, NDUST, NPRO, 1, NPRO, xmap)[:, 0, :] / area_star * 100.
    i = int(np.argmax(depth))
    print("transit depth %.4f .. %.4f per cent over %d wavenumbers; deepest at %.1f cm-1" % (depth.min(), depth.max(), W, WAVE[i]))
    print("transmission of the lowest / highest tangent path there: %.3e / %.6f" % (TRANS[i, 0], TRANS[i, -1]))
    print("d depth / d T(level) there, largest at level %d: %.3e per cent / K" % (int(np.argmax(np.abs(ddepth[i]))), np.abs(ddepth[i]).max()))
    print("k_transit_sens %.3f ms, k_transit_grad %.3f ms, %.1f MB of scratch beyond the gas stage (dSPECOUT would be %.1f MB)"
          % (ms_sens, ms_grad, scratch / 1e6, 8e-6 * W * NPAR * 2 * L * P))
    eng.close()


if __name__ == "__main__":
    main()
