#!/usr/bin/env python
"""Aerosol optical properties of one size distribution on the GPU: what Scatter_0.makephase (Mie theory integrated over a
log-normal distribution of radii) returns, from the engine directly -- no reference needed.

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
    phas /= 4.0 * np.pi                                         # as the class method normalises it
    print("angles (deg):", thetax)
    for i, w in enumerate(wavel):
        print("lambda %.1f um: %d radii  k_ext %.3e cm2  albedo %.4f  P(0) %.3f  P(180) %.4f"
              % (w, counts[i], xext[i], xscat[i] / xext[i], phas[i, 0], phas[i, -1]))
    ms, blocks, radii = eng.mie_last()
    print("kernels: %.2f ms in %d block(s) of %d radii" % (ms, blocks, radii))
    eng.close()


if __name__ == "__main__":
    main()
