"""Geometry of the disc-averaged forward model with gradients (nemesisdiscfmg, ForwardModel_0.py:1719-1834) in the form the fused
engine call `AnsfmEngine.cirsradg_ck_disc` takes it: the weighted sum over the averaging points of a geometry (:1789-1794) as a
mixing matrix, and the test that the points are paths through one layer sequence that differ in SCALE only.

calc_pathg sets LAYANG = 0 for every point with an emission angle >= 0 (:3118), so such points share their layers and the layers
their paths include; the emission angle enters through SCALE alone.  `shared_sequence` does not rely on that: it compares what
the points hold, bit for bit, and declines otherwise."""
import numpy as np


def average_mix(WGEOM_row):
    """WGEOM[IGEOM, :NAV] -> C (1, NAV): the sum of :1789-1794 as the mixing matrix of one geometry"""
    return np.ascontiguousarray(np.asarray(WGEOM_row, dtype=np.float64).reshape(1, -1))


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_LAYER_FIELDS = ("PRESS", "TEMP", "AMOUNT", "DTE", "DAM", "DCO")
_PATH_FIELDS = ("NLAYIN", "LAYINC", "EMTEMP")


def shared_sequence(points):
    """points: per averaging point the record (LayerX, PathX, SurfaceX, xmap) as process_IAV leaves them after calc_pathg
    (:2004-2036).  -> LAYINC (N,) int32, EMTEMP (N,), SCALE (N, NAV) when every point has one path (NPATH = 1) and the points agree
    bit for bit in LayerX.PRESS / TEMP / AMOUNT / DTE / DAM / DCO, PathX.NLAYIN / LAYINC / EMTEMP, SurfaceX.TSURF and xmap; else
    None."""
    if not points:
        return None
    L0, P0, S0, x0 = points[0]
    for L, P, S, xmap in points:
        if int(P.NPATH) != 1:
            return None
    for L, P, S, xmap in points[1:]:
        if not all(_same_bits(getattr(L, f), getattr(L0, f)) for f in _LAYER_FIELDS):
            return None
        if not all(_same_bits(getattr(P, f), getattr(P0, f)) for f in _PATH_FIELDS):
            return None
        if not _same_bits(np.float64(S.TSURF), np.float64(S0.TSURF)) or not _same_bits(xmap, x0):
            return None
    N = int(np.asarray(P0.NLAYIN).reshape(-1)[0])
    LAYINC = np.ascontiguousarray(np.asarray(P0.LAYINC).reshape(-1, 1)[:N, 0], dtype=np.int32)
    EMTEMP = np.ascontiguousarray(np.asarray(P0.EMTEMP, dtype=np.float64).reshape(-1, 1)[:N, 0])
    SCALE = np.ascontiguousarray(np.stack([np.asarray(P.SCALE, dtype=np.float64).reshape(-1, 1)[:N, 0] for _, P, _, _ in points], axis=1))
    return LAYINC, EMTEMP, SCALE
