"""Geometry of the solar-occultation forward model with gradients (nemesisSOfmg, ForwardModel_0.py:983-1249) in the form the
fused engine call `AnsfmEngine.cirsradg_ck_occultation` takes it: the interpolation of the limb paths to the tangent heights
of the measurement (:1208-1232) as a mixing matrix C (NGEOM, NPATH), MOD = SPECOUT @ C.T."""
import numpy as np

from .transit import tangent_heights_km  # noqa: F401  (BASEH_TANHE of :1180-1182 is the transit's :1906-1908)


def tangent_mix(BASEH_TANHE_km, TANHE):
    """C (NGEOM, NPATH) of nemesisSOfmg :1211-1232 as it stands.  BASEH_TANHE_km (NPATH,): the tangent height of every path in
    km; TANHE (NGEOM,) or (NGEOM, NAV): Measurement.TANHE, of which the first averaging point counts.  The path nearest to the
    tangent height and its neighbour on the other side get the weights (1 - fhl) and (1 - fhh); a lower neighbour of -1 (a
    tangent height below the lowest path) is the LAST path, as the reference's Python index is; above the top path the lower
    neighbour gets weight 1.  (nemesisSOfm :947 divides the nearest height by 1e3 once more before comparing; this method does
    not, and `jacobian_dropin._ansfm_limb_to_tangent_heights` keeps that other form: the two are not shared.)"""
    B = np.asarray(BASEH_TANHE_km, dtype=np.float64).reshape(-1)
    T = np.asarray(TANHE, dtype=np.float64)
    T = T.reshape(T.shape[0], -1)[:, 0]
    P = B.size
    C = np.zeros((T.size, P))
    for i in range(T.size):
        ibase = int(np.argmin(np.abs(B - T[i])))                   # :1214
        base0 = B[ibase]                                           # :1215, no second / 1e3
        if base0 <= T[i]:
            ibasel, ibaseh = ibase, ibase + 1
        else:
            ibasel, ibaseh = ibase - 1, ibase
        if ibaseh > P - 1:                                         # :1224-1226
            C[i, ibasel] += 1.0
        else:
            fhl = (T[i] - B[ibasel]) / (B[ibaseh] - B[ibasel])     # B[-1]: the last path
            fhh = (B[ibaseh] - T[i]) / (B[ibaseh] - B[ibasel])
            C[i, ibasel % P] += 1. - fhl
            C[i, ibaseh] += 1. - fhh
    return C
