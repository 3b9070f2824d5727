"""Aerosol phase functions on the calculation grid (Scatter_0.calc_phase :760, calc_hgphase :699, interp_phase :732,
calc_lpphase :1060, legendre_p :2224, calc_phase_ray :834): the cases of tests/golden/phase.npz
(tools/golden/gen_golden_phase.py runs the reference on them) and the project's own NumPy restatement -- the written-down
contract of the kernels in csrc/ansfm_phase_kernels.hip.h.

calc_phase(Theta [nth], Wave [W]) -> (W, nth, NDUST):
  * phase1 (NWS, nth, NDUST) on Scatter.WAVE
      IMIE 0  c = cos(Theta / 180. * pi); t_k = (1 - G_k G_k) / (1 - 2 G_k c + G_k G_k) ** 1.5;
              (F t1 + (1 - F) t2) / (4 pi)      (NumPy evaluates `** 2.` as a product)
      IMIE 1  interp1d(THETA, PHASE, axis=1)(Theta)
      IMIE 2  sum over l = 0 .. NLPOL - 1, ascending from 0.0, of P_l(c) WLPOL[:, l, :];
              P_n = ((2 n - 1) c P_{n-1} - (n - 1) P_{n-2}) / n
  * interp1d(WAVE, phase1, axis=0, fill_value='extrapolate')(Wave)
Both interpolations are scipy's interp1d._call_linear (`lin` below).  `tab` is what ansfm_calc_phase takes: IMIE 0 the stack
(F, G1, G2) as (3, NWS, NDUST), IMIE 1 PHASE (NWS, NTAB, NDUST), IMIE 2 WLPOL (NWS, NLPOL, NDUST).

`ulp`: an object called on the result of every cos and pow -- the identity for the restatement itself; brdf_cases.Nudge moves
each result by one np.nextafter to measure what one ulp in those is worth."""
import numpy as np

from brdf_cases import PATTERNS, Exact, Nudge  # noqa: F401  (re-exported for the generator and the tests)

PI = np.pi
_same = Exact()
THETA41 = np.linspace(0.0, 180.0, 41)
EXACT_KINDS = (1,)              # IMIE modes without cos or pow: held to the reference bit for bit


def lin(x, y, xn):
    """interp1d._call_linear along axis 0 of y (scipy 1.15.3): the end intervals extrapolate"""
    x, y, xn = np.asarray(x, float), np.asarray(y, float), np.asarray(xn, float)
    hi = np.clip(np.searchsorted(x, xn, "left"), 1, len(x) - 1).astype(int)
    lo = hi - 1
    ex = (slice(None),) + (None,) * (y.ndim - 1)
    slope = (y[hi] - y[lo]) / (x[hi] - x[lo])[ex]
    return slope * (xn - x[lo])[ex] + y[lo]


def legendre_p(l, x):
    if l == 0:
        return np.ones_like(x)
    p0, p1 = np.ones_like(x), x
    for n in range(2, l + 1):
        p0, p1 = p1, ((2 * n - 1) * x * p1 - (n - 1) * p0) / n
    return p1


def phase1_np(imie, ttab, tab, theta, ulp=_same):
    """(NWS, nth, NDUST) on the aerosol grid"""
    theta, tab = np.asarray(theta, float), np.asarray(tab, float)
    if imie == 1:
        ttab = np.asarray(ttab, float)
        if theta.min() < ttab[0] or theta.max() > ttab[-1]:
            raise ValueError("A value in x_new is outside the interpolation range.")
        return np.moveaxis(lin(ttab, np.moveaxis(tab, 1, 0), theta), 0, 1)
    c = ulp.unit(np.cos(theta / 180. * PI))
    if imie == 0:
        F, G1, G2 = (a[:, None, :] for a in tab)
        cx = c[None, :, None]
        t1 = (1. - G1 * G1) / ulp((1. - 2. * G1 * cx + G1 * G1) ** 1.5)
        t2 = (1. - G2 * G2) / ulp((1. - 2. * G2 * cx + G2 * G2) ** 1.5)
        return (F * t1 + (1.0 - F) * t2) / (4.0 * PI)
    out = np.zeros((tab.shape[0], theta.shape[0], tab.shape[2]))
    for l in range(tab.shape[1]):
        out += legendre_p(l, c)[None, :, None] * tab[:, l, None, :]
    return out


def covers(swave, wave):
    """calc_phase's range test (:790)"""
    swave, wave = np.asarray(swave, float), np.asarray(wave, float)
    return not (swave.min() > (1. + 1.0e-6) * wave.min() or swave.max() < (1. - 1.0e-6) * wave.max())


def calc_phase_np(imie, swave, ttab, tab, theta, wave, ulp=_same):
    if not covers(swave, wave):
        raise ValueError("Aerosol wavelength range does not fully cover the calculation wavelength range")
    return lin(swave, phase1_np(imie, ttab, tab, theta, ulp), wave)


def calc_phase_ray_np(theta, ulp=_same):
    c = ulp.unit(np.cos(np.asarray(theta, float) / 180. * PI))
    return 0.75 * (1.0 + c * c) / (4.0 * PI)


def hg_on_grid(swave, tab, wave):
    """f_w, g1_w, g2_w (3, NDUST, W): np.interp of F, G1, G2 (ForwardModel_0.py:5131-5133)"""
    return np.array([[np.interp(wave, swave, tab[k][:, d]) for d in range(tab.shape[2])] for k in range(3)])


def phasarr_np(imie, swave, ttab, tab, theta, wave, ulp=_same):
    """PHASE_ARRAY[:, :, :, ::-1] of ForwardModel_0.py:5128-5142, (NDUST, W, 2, nth)"""
    theta, tab = np.asarray(theta, float), np.asarray(tab, float)
    nd, W, nth = tab.shape[2], len(wave), len(theta)
    arr = np.zeros((nd, W, 2, nth))
    if imie == 0:
        hg = hg_on_grid(swave, tab, wave)
        arr[:, :, 0, -1], arr[:, :, 0, -2], arr[:, :, 0, -3] = hg[0], hg[1], hg[2]
    else:
        arr[:, :, 0, :] = np.transpose(calc_phase_np(imie, swave, ttab, tab, theta, wave, ulp), (2, 0, 1))
    arr[:, :, 1, :] = np.cos(theta * np.pi / 180)
    return np.ascontiguousarray(arr[:, :, :, ::-1])


def deviation(got, ref):
    """largest |got - ref| relative to the column maximum over the angles (axis 1 of (W, nth, NDUST); a ray: the maximum)"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    scale = np.abs(ref).max(axis=1, keepdims=True) if ref.ndim == 3 else np.abs(ref).max()
    return float(np.max(np.abs(got - ref) / scale))


INPUTS = ("imie", "swave", "ttab", "tab", "theta", "wave")


def _case(imie, swave, ttab, tab, theta, wave):
    f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return {"imie": np.asarray(int(imie)), "swave": f(swave), "ttab": f(ttab), "tab": f(tab), "theta": f(theta), "wave": f(wave)}


def _hg_tab(rng, nws, nd, gmax=0.9):
    F = rng.uniform(0.05, 0.95, (nws, nd))
    G1 = rng.uniform(0.1, gmax, (nws, nd))
    G2 = -rng.uniform(0.1, 0.6, (nws, nd))
    return np.array([F, G1, G2])


def _mie_tab(rng, nws, ttab, nd):
    """forward-peaked positive tabulated phase functions"""
    c = np.cos(np.asarray(ttab) / 180. * PI)[None, :, None]
    g = rng.uniform(0.2, 0.85, (nws, 1, nd))
    return (1. - g * g) / (1. - 2. * g * c + g * g) ** 1.5 / (4. * PI) * rng.uniform(0.9, 1.1, (nws, len(ttab), nd))


def _lp_tab(rng, nws, nl, nd):
    """Legendre weights of a Henyey-Greenstein function, (2 l + 1) g^l / (4 pi), perturbed"""
    l = np.arange(nl)[None, :, None]
    g = rng.uniform(0.3, 0.8, (nws, 1, nd))
    return (2 * l + 1) * g ** l / (4. * PI) * rng.uniform(0.95, 1.05, (nws, nl, nd))


def golden_cases():
    """name -> inputs; `ray`: theta only"""
    rng = np.random.default_rng(20261021)
    out = {}
    # both grid ends, one point 5e-7 (relative) outside each end (extrapolation inside the range test's tolerance), one interior
    sw = np.array([800.0, 1250.0])
    out["hg-2x1"] = _case(0, sw, [], _hg_tab(rng, 2, 1), [0.0, 90.0, 180.0],
                          [sw[0] * (1 - 5e-7), sw[0], 1000.3, sw[1], sw[1] * (1 + 5e-7)])
    # seven populations, a 64-lane tail; g1 up to 0.999, one g = 0, F in {0, 1} among the rows
    sw = np.array([400.0, 650.0, 900.5, 1400.0, 2100.0])
    tab = _hg_tab(rng, 5, 7)
    tab[1][:, 0] = [0.9, 0.99, 0.999, 0.5, 0.95]
    tab[1][2, 3] = 0.0; tab[2][3, 4] = 0.0
    tab[0][0, 1] = 0.0; tab[0][4, 2] = 1.0; tab[0][2, 5] = 1.0; tab[0][1, 6] = 0.0
    wave = np.sort(np.concatenate([sw, rng.uniform(sw[0], sw[-1], 62)]))
    out["hg-7pop"] = _case(0, sw, [], tab, THETA41, wave)
    # tabulated: every node, 0 and 180, midpoints; W on every node and between
    sw = np.array([1000.0, 1100.0, 1300.0, 1350.0])
    tt = np.array([0.0, 30.0, 75.0, 120.0, 180.0])
    th = np.sort(np.concatenate([tt, 0.5 * (tt[1:] + tt[:-1])]))
    out["mie-nodes"] = _case(1, sw, tt, _mie_tab(rng, 4, tt, 2), th,
                             np.sort(np.concatenate([sw, 0.5 * (sw[1:] + sw[:-1]), [1000.0 + 1e-9, 1349.999]])))
    # the single-scattering shape: 4 path angles
    sw = np.linspace(2000.0, 2400.0, 9)
    out["mie-paths"] = _case(1, sw, THETA41, _mie_tab(rng, 9, THETA41, 3), [12.25, 90.0, 133.7, 179.5],
                             np.linspace(2000.0, 2400.0, 130))
    for nl in (1, 2, 36):                    # recurrence not entered / entered once / 36 moments
        sw = np.array([500.0, 700.0, 1000.0])
        out[f"lp-{nl}"] = _case(2, sw, [], _lp_tab(rng, 3, nl, 2), THETA41, np.linspace(500.0, 1000.0, 70))
    out["ray"] = {"theta": np.array([0.0, 33.3, 90.0, 170.0, 180.0])}
    # a wavelength grid (ISPACE 1: ascending micrometres)
    sw = np.array([0.4, 0.7, 1.0, 2.5, 5.0])
    out["um"] = _case(0, sw, [], _hg_tab(rng, 5, 2), THETA41[::4], np.linspace(0.45, 4.8, 33))
    return out


def load_golden(path):
    """name -> dict of the arrays of one case (inputs, ref, ulp)"""
    z = np.load(path)
    out = {}
    for key in z.files:
        name, field = key.split("__")
        out.setdefault(name, {})[field] = z[key]
    return out


def evaluate_np(d, ulp=_same):
    if "imie" not in d:
        return calc_phase_ray_np(d["theta"], ulp)
    return calc_phase_np(int(d["imie"]), d["swave"], d["ttab"], d["tab"], d["theta"], d["wave"], ulp)
