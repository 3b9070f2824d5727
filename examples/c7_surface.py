#!/usr/bin/env python
"""A Hapke surface under a scattering atmosphere, on the GPU from end to end: the surface's BRDF matrix (what
ForwardModel_0.calc_brdf_matrix builds: the BRDF integrated over azimuth against cos(ic phi), for every pair of quadrature
angles) and then the multiple-scattering core with that matrix as its lower boundary (lowbc = 2) -- no reference needed.

    python examples/c7_surface.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import archnemesis_dist_amd as pkg


def main():
    eng = pkg.AnsfmEngine(0)
    W, NMU, NPHI, NF, NLAY = 8, 5, 101, 4, 6
    wave = np.linspace(4000.0, 4700.0, W)                       # cm-1
    x, wt = np.polynomial.legendre.leggauss(NMU)
    MU, WTMU = 0.5 * (x + 1.0), 0.5 * wt                        # quadrature cosines, ascending as Scatter_0 stores them
    # a synthetic regolith: albedo rising with wavenumber; w, K, BS0, hs, BC0, hc, ROUGHNESS, G1, G2, F
    one = np.ones(W)
    params = np.stack([np.linspace(0.3, 0.8, W), 1.2 * one, 0.8 * one, 0.06 * one, 0.3 * one, 0.1 * one, 20.0 * one,
                       -0.3 * one, 0.4 * one, 0.6 * one])
    brdf = eng.brdf_matrix(2, params, MU, NPHI, NF)             # (W, NMU, NMU, NF + 1)
    print("BRDF matrix %s in %.3f ms of kernel time; plane 0 at normal incidence and emission: %s"
          % (brdf.shape, eng.brdf_last(), np.array2string(brdf[:, 0, 0, 0], precision=4)))
    # the same surface seen at three geometries of a measurement (solar zenith, emission, azimuth; 180 = backscattering)
    pts = eng.surface_brdf(2, params, [30.0, 30.0, 60.0], [30.0, 10.0, 45.0], [180.0, 90.0, 0.0])
    print("BRDF at opposition / off-axis / forward, first wavenumber:", np.array2string(pts[0], precision=4))
    # a thin hazy atmosphere above it: Henyey-Greenstein aerosol (imie = 0), no thermal emission, unit solar flux
    phasarr = np.zeros((1, W, 2, 3))
    phasarr[0, :, 0, :3] = [0.7, 0.6, -0.3]                     # f, g1, g2
    phasarr[0, :, 1, :] = [-1.0, 0.0, 1.0]
    taus = np.full((W, 1, NLAY), 0.03); omegas = np.full((W, 1, NLAY), 0.7)
    zero = np.zeros((W, NLAY))
    rad = eng.scloud11wave_core(phasarr, np.zeros((W, NMU)), [35.0], [20.0], one, [60.0], 2, brdf, MU, WTMU, NF, wave, zero, taus,
                                zero, omegas, NPHI, 0, 0, np.ones((W, 1, NLAY)))
    dark = eng.scloud11wave_core(phasarr, np.zeros((W, NMU)), [35.0], [20.0], one, [60.0], 2, np.zeros_like(brdf), MU, WTMU, NF,
                                 wave, zero, taus, zero, omegas, NPHI, 0, 0, np.ones((W, 1, NLAY)))
    for w in range(W):
        print("%.0f cm-1: w = %.2f  reflected radiance per unit solar flux %.5f  (over a black surface %.5f)"
              % (wave[w], params[0, w], rad[0, 0, w], dark[0, 0, w]))
    eng.close()


if __name__ == "__main__":
    main()
