#!/usr/bin/env python
"""Aerosol optical properties of one size distribution on the GPU: what Scatter_0.makephase (Mie theory integrated over a
log-normal distribution of radii) returns, from the engine directly -- no reference needed -- and the double
Henyey-Greenstein parameters the class method fits to its phase functions when IMIE = 0 (Scatter_0.subfithgm).

    python examples/c6_mie.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import archnemesis_dist_amd as pkg


def main():
    eng = pkg.AnsfmEngine(0)
    wavel = np.array([0.5, 1.0, 2.0, 4.0])                      # um
    refindx = np.tile([1.4, 0.01], (wavel.shape[0], 1))         # m = 1.4 - 0.01i
    theta = np.array([0.0, 10.0, 30.0, 60.0, 90.0])             # the angles beyond 90 degrees come back mirrored
    dsize = np.array([0.5, 0.3, 0.0])                           # log-normal: r0 = 0.5 um, sigma = 0.3
    rs = np.array([0.015 * wavel.min(), 0.0, 0.015 * wavel.min()])   # open range: ends where n(r) Q_sca has died away
    xscat, xext, thetax, phas, counts = eng.mie_makephase(wavel, 2, dsize, rs, refindx, theta, return_counts=True)
    f, g1, g2, rms, calls = eng.hg_fit(thetax, phas, return_counts=True)   # subfithgm takes the phase function normalised to 4 pi
    phas /= 4.0 * np.pi                                         # as the class method normalises it
    print("angles (deg):", thetax)
    for i, w in enumerate(wavel):
        print("lambda %.1f um: %d radii  k_ext %.3e cm2  albedo %.4f  P(0) %.3f  P(180) %.4f"
              % (w, counts[i], xext[i], xscat[i] / xext[i], phas[i, 0], phas[i, -1]))
        print("    double Henyey-Greenstein fit: f %.4f  g1 %.4f  g2 %.4f  rms %.3f  (%d calls of mrqminl, %d accepted)"
              % (f[i], g1[i], g2[i], rms[i], calls[i, 0], calls[i, 1]))
    ms, blocks, radii = eng.mie_last()
    print("kernels: %.2f ms in %d block(s) of %d radii; the fits %.2f ms" % (ms, blocks, radii, eng.hg_fit_last()))
    eng.close()


if __name__ == "__main__":
    main()
