"""Geometry of the primary-transit forward model (nemesisPTfm, ForwardModel_0.py:1838-1995) in the form the fused engine call
`AnsfmEngine.cirsradg_ck_transit` takes it: the tangent height of every limb path and the weights that turn the path
transmissions into the absorbing area, AREA = sum_p c_p (1 - T_p)."""
import numpy as np


def tangent_heights_km(BASEH, NLAYIN, LAYINC):
    """BASEH_TANHE of :1906-1908: the base height (km) of the layer in the middle of every path."""
    BASEH = np.asarray(BASEH, dtype=np.float64)
    NLAYIN = np.asarray(NLAYIN).reshape(-1)
    LAYINC = np.asarray(LAYINC).reshape(-1, NLAYIN.size)
    return np.array([BASEH[LAYINC[int(NLAYIN[i] / 2), i]] / 1.0e3 for i in range(NLAYIN.size)])


def path_weights(tanhe_km, RADIUS):
    """c_p of the trapezoid of :1949-1954, sum_i 0.5 (S_i + S_{i+1}) dH_i with S_i = (1 - T_i) 2 pi (h_i + RADIUS), collected
    by path: c_p = 2 pi (h_p + RADIUS) 0.5 (dH_{p-1} [p > 0] + dH_p [p < P - 1]); heights as the reference forms them."""
    t = np.asarray(tanhe_km, dtype=np.float64)
    dH = (t[1:] - t[:-1]) * 1.0e3
    half = np.zeros(t.size)
    half[:-1] += 0.5 * dH
    half[1:] += 0.5 * dH
    return 2. * np.pi * (t * 1.0e3 + RADIUS) * half
