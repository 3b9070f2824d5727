#!/usr/bin/env python
"""An unresolved planet on the GPU from end to end: the disc-averaged thermal emission and its gradient with respect to a
temperature profile and to the surface temperature, from a synthetic k-table atmosphere -- what nemesisdiscfmg computes, with
the averaging points (emission angles over the disc) mixed on the device before anything of the size of one dSPECOUT
(NWAVE, NPAR, NLAYIN, 1) per point exists.  No reference needed.

    python examples/c11_disc.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import archnemesis_dist_amd as pkg
from archnemesis_dist_amd import synthetic as syn, disc


def main():
    eng = pkg.AnsfmEngine(0)
    W, G, S, L, NPRO = 512, 10, 3, 40, 40
    PRESS, TEMP, K = syn.synth_ktable(W, G, 8, 6, S, seed=1)
    WAVE = 600.0 + 0.5 * np.arange(W)
    eng.upload_ktable(K, PRESS, TEMP, WAVE, syn.gauss_legendre_01(G)[1])
    atm = syn.synth_atmosphere(L, S, seed=2)
    lp, lt, am = atm["lay_press_pa"][0], atm["lay_temp"][0], atm["amount"][0]        # layer 0 the deepest
    # five averaging points: Gauss-Legendre nodes in mu = cos(emission angle) over the disc, weights 2 mu dmu
    mu, wt = syn.gauss_legendre_01(5)
    WGEOM = 2.0 * mu * wt
    WGEOM = WGEOM / WGEOM.sum()
    # every point looks down through the same layers, from the top one to the ground; only the slant factor differs
    LAYINC = np.arange(L - 1, -1, -1).astype(np.int32)
    EMTEMP = lt[LAYINC]
    SCALE = np.ascontiguousarray(np.repeat((1.0 / mu)[None, :], L, axis=0))           # (N, NAV)
    TSURF, EMISSIVITY = 350.0, np.linspace(0.9, 0.7, W)
    NVMR, NDUST = S, 0
    NPAR = NVMR + 2 + NDUST
    MOD, SPEC, dTSMOD, _ = eng.cirsradg_ck_disc(0, lp, lt, am, None, None, NVMR, NPAR, np.arange(S, dtype=np.int32), LAYINC, SCALE, EMTEMP,
                                                TSURF, EMISSIVITY=EMISSIVITY, mix=disc.average_mix(WGEOM), gradients_on_device=True)
    scratch, ms_sens, ms_grad = eng.disc_last()
    # layers -> levels -> state vector on the device: one layer per level here, the state vector is the temperature profile
    eye = np.eye(L, NPRO)
    xmap = np.zeros((NPRO, NPAR, NPRO)); xmap[np.arange(NPRO), NVMR, np.arange(NPRO)] = 1.0
    eng.map2pro(None, W, NVMR, NDUST, NPRO, 1, np.array([L]), np.arange(L)[:, None], eye, eye, eye, INCPAR=[NVMR], to_host=False)
    dmod = eng.map2xvec(None, W, NVMR, NDUST, NPRO, 1, NPRO, xmap)[:, 0, :]           # (W, NPRO)
    i = int(np.argmax(MOD[:, 0]))
    lev = int(np.argmax(np.abs(dmod[i])))
    print("disc average of %d points (emission angles %s deg): radiance %.3e .. %.3e W cm-2 sr-1 (cm-1)-1, brightest at %.1f cm-1"
          % (mu.size, np.array2string(np.degrees(np.arccos(mu)), precision=1), MOD.min(), MOD.max(), WAVE[i]))
    print("limb darkening there: the point nearest the limb is %.3f of the point nearest the centre" % (SPEC[i, 0] / SPEC[i, -1]))
    print("d R / d T(level) there largest at level %d: %.3e / K;  d R / d TSURF %.3e / K" % (lev, dmod[i, lev], dTSMOD[i, 0]))
    print("k_disc_planck + k_disc_sens %.3f ms, k_disc_grad %.3f ms, %.2f MB of scratch beyond the gas stage, dMOD %.2f MB (the %d "
          "dSPECOUT arrays would be %.2f MB)" % (ms_sens, ms_grad, scratch / 1e6, 8e-6 * W * NPAR * L, mu.size, 8e-6 * W * NPAR * L * mu.size))
    eng.close()


if __name__ == "__main__":
    main()
