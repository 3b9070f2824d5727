"""Pseudo-continuum of the weak lines (LineData_0.add_pseudo_continuum_monochromatic_absorption, LineData_0.py:486): the
seeded synthetic bin sets of tests/golden/lbl_pseudo_continuum.npz (tools/golden/gen_golden_lbl_pc.py runs the reference
on them) and a NumPy restatement in the form the kernels have -- every sum gathered by its owner, in the reference's order.
tests/test_lbl_pc_restatement.py holds the restatement to the reference's results bit for bit; the GPU tests use it as
the checker at sizes the reference's Python loops do not reach."""
import numpy as np
from scipy.special import voigt_profile

C_LIGHT, H_PLANCK, K_BOLTZ, N_AVOGADRO = 2.99792458E10, 6.62607015E-27, 1.380649E-16, 6.02214129E+23
C2 = C_LIGHT * H_PLANCK / K_BOLTZ
VOIGT, LORENTZ, GAUSSIAN = 0, 4, 12          # SpectroscopicLineProfileEnum values
SHAPE_NAMES = {VOIGT: "voigt", LORENTZ: "lorentz", GAUSSIAN: "gaussian"}
INPUTS = ("wn_grid", "t_calc", "t_ref", "p_calc", "p_ref", "q_ratio", "isotopic_abundance", "isotopic_mass", "mol_mix_frac",
          "bparams", "centers", "widths", "sw_sum", "e_lower", "out0", "lineshape_id", "n_neighbour_bins")
COVERING = ("regular", "overlapping", "fine_bins", "lorentz", "gaussian", "one_neighbour", "onto_nonzero", "two_broadeners",
            "three_broadeners")   # bins from below the grid to above it: the reference leaves one grid point (the last) at zero


def lineshape(lid, dwn, alpha_d, gamma_l):
    if lid == LORENTZ:
        return gamma_l / (np.pi * (gamma_l ** 2 + dwn ** 2))
    if lid == GAUSSIAN:
        return np.sqrt(np.log(2) / np.pi) / alpha_d * np.exp(-(dwn ** 2 * np.log(2)) / (alpha_d ** 2))
    return voigt_profile(dwn, alpha_d / np.sqrt(2.0 * np.log(2.0)), gamma_l)


def bin_params(t_calc, t_ref, p_calc, p_ref, q_ratio, isotopic_mass, mol_mix_frac, bparams, centers, sw_sum, e_lower):
    """store (3, N): strength, alpha_d, gamma_l (:521-553), element by element like the reference's loops"""
    N = centers.shape[0]
    store = np.zeros((3, N))
    boltz = C2 * (t_calc - t_ref) / (t_calc * t_ref)
    dconst = (1.0 / C_LIGHT) * np.sqrt(2 * np.log(2) * N_AVOGADRO * K_BOLTZ)
    t_ratio, p_ratio = t_ref / t_calc, p_calc / p_ref
    for i in range(N):
        stim_ref = 1 - np.exp(-C2 * centers[i] / t_ref)
        store[0, i] = sw_sum[i] * ((1 - np.exp(-C2 * centers[i] / t_calc)) / stim_ref) * np.exp(boltz * e_lower[i]) * q_ratio
        store[1, i] = dconst * centers[i] * np.sqrt(t_calc / isotopic_mass)
        g = 0
        for j in range(mol_mix_frac.shape[0]):
            g += (t_ratio ** bparams[3 * j + 1, i]) * bparams[3 * j, i] * mol_mix_frac[j] * p_ratio
        store[2, i] = g
    return store


def geometry(wn_grid, centers, widths):
    """first, last (:399-416), the largest touched grid point (j_max, :463; 0 if none) and the largest width"""
    N, nw = centers.shape[0], wn_grid.shape[0]
    first = last = -1
    jmax = 0
    for i in range(N):
        c, w = centers[i], widths[i]
        if first == -1 and c - w / 2.0 <= wn_grid[0]:
            first = i
        if last == -1 and c + w / 2.0 > wn_grid[-1]:
            last = i
        a, b = 0, nw                      # first j with (wn_j - c)/w >= 0.5: the expression does not decrease along the grid
        while a < b:
            mid = (a + b) // 2
            if (wn_grid[mid] - c) / w < 0.5:
                a = mid + 1
            else:
                b = mid
        if a > 0 and (wn_grid[a - 1] - c) / w >= -0.5:
            jmax = max(jmax, a - 1)
    return (N if first == -1 else first), (N if last == -1 else last), jmax, float(np.max(widths))


def spread(lid, centers, widths, store, first, last, nb):
    """store_x (N,): shapes and their sum per source bin, then each target bin adds its sources in ascending order"""
    N = centers.shape[0]
    y = np.zeros((N, 2 * nb + 1))
    s = np.zeros(N)
    for i in range(first, last):
        tot = 0.0
        for k in range(2 * nb + 1):
            ii = i + k - nb
            if 0 <= ii < N:
                y[i, k] = lineshape(lid, centers[ii] - centers[i], store[1, i], store[2, i])
                tot += y[i, k]
        s[i] = tot
    x = np.zeros(N)
    for t in range(N):
        v = 0.0
        for i in range(max(t - nb, first, 0), min(t + nb, last - 1, N - 1) + 1):
            if s[i] != 0:
                v += store[0, i] * y[i, t - i + nb] / s[i]
        x[t] = v / widths[t]
    return x, y


def interpolate(wn_grid, centers, widths, x, factor, jmax, wmax, out, j_from=0, j_to=None):
    """out[j] += z0/z1 for the grid points j_from <= j < min(j_to, jmax): each point adds its bins in ascending order"""
    N = centers.shape[0]
    lo = centers - widths / 2.0
    j_to = wn_grid.shape[0] if j_to is None else j_to
    for j in range(j_from, min(j_to, jmax)):
        wn = wn_grid[j]
        margin = 1e-9 * (abs(wn) + wmax)
        ilo = int(np.searchsorted(lo, wn - wmax - margin, side="left"))
        ihi = int(np.searchsorted(lo, wn + margin, side="right"))
        z0, z1 = 0.0, 0.0
        for i in range(ilo, ihi):
            delta = (wn - centers[i]) / widths[i]
            if delta < -0.5 or delta >= 0.5:
                continue
            n = 1.0 - np.abs(delta)
            if delta < 0 and i > 0:
                z0 += (1 - n) * factor * x[i - 1]
            elif delta > 0 and i < N - 1:
                z0 += (1 - n) * factor * x[i + 1]
            z0 += n * factor * x[i]
            z1 += 1.0
        if z1 != 0.0:
            out[j] += z0 / z1


def pseudo_continuum_np(wn_grid, lineshape_id, t_calc, t_ref, p_calc, p_ref, q_ratio, isotopic_abundance, isotopic_mass,
                        mol_mix_frac, bparams, centers, widths, sw_sum, e_lower, out, n_neighbour_bins=3, j_from=0, j_to=None):
    """The reference's call for one (T, p) point: adds to out (nw,) -- only to the points j_from <= j < j_to when given --
    and returns store (3, N) and store_x (N,).  The lower bin edges must be ascending."""
    assert np.all(widths > 0) and np.all(np.diff(centers - widths / 2.0) >= 0)
    store = bin_params(float(t_calc), float(t_ref), float(p_calc), float(p_ref), float(q_ratio), float(isotopic_mass),
                       mol_mix_frac, bparams, centers, sw_sum, e_lower)
    first, last, jmax, wmax = geometry(wn_grid, centers, widths)
    x, _ = spread(int(lineshape_id), centers, widths, store, first, last, int(n_neighbour_bins))
    interpolate(wn_grid, centers, widths, x, float(isotopic_abundance), jmax, wmax, out, j_from, j_to)
    return store, x


# ---- seeded synthetic bins ------------------------------------------------------------------------------------------------
def synth_bins(rng, centers, widths, M=1):
    """weak-line sums of the bins: strengths over five decades, lower-state energies, (gamma, n, delta) per broadener"""
    N = centers.shape[0]
    bp = np.zeros((3 * M, N))
    for j in range(M):
        bp[3 * j] = rng.uniform(0.02, 0.1, N); bp[3 * j + 1] = rng.uniform(0.4, 0.8, N); bp[3 * j + 2] = rng.uniform(-0.01, 0.01, N)
    mmf = rng.uniform(0.2, 1.0, M)
    return dict(centers=np.ascontiguousarray(centers, dtype=float), widths=np.ascontiguousarray(widths, dtype=float),
                sw_sum=10.0 ** rng.uniform(-27, -22, N), e_lower=rng.uniform(0.0, 2500.0, N), bparams=bp,
                mol_mix_frac=mmf / mmf.sum())


def regular_bins(lo, hi, width):
    n = int(round((hi - lo) / width))
    return lo + width * (np.arange(n) + 0.5), np.full(n, float(width))


def golden_cases():
    """name -> inputs of the reference's call (INPUTS), in a fixed order and from fixed seeds"""
    grid = np.linspace(1000.0, 1100.0, 1001)
    cases = {}

    def add(name, seed, cw, lid=VOIGT, nb=3, M=1, wn_grid=grid, out0=None, t=(180.0, 0.3, 1.7)):
        rng = np.random.default_rng(seed)
        d = synth_bins(rng, cw[0], cw[1], M)
        d.update(wn_grid=wn_grid, t_calc=t[0], t_ref=296.0, p_calc=t[1], p_ref=1.0, q_ratio=t[2], isotopic_abundance=0.93,
                 isotopic_mass=28.0, lineshape_id=lid, n_neighbour_bins=nb,
                 out0=np.zeros(wn_grid.shape[0]) if out0 is None else out0)
        cases[name] = d

    add("regular", 1, regular_bins(990.0, 1110.0, 1.0))
    rng = np.random.default_rng(2)            # jittered centres and widths: gaps and overlaps, lower edges ascending
    lo = 989.0 + np.cumsum(rng.uniform(0.7, 1.3, 125)); w = rng.uniform(0.6, 1.4, 125)
    add("jittered", 3, (lo + w / 2.0, w), t=(140.0, 0.05, 2.4))
    lo = 985.0 + 1.0 * np.arange(130)
    add("overlapping", 4, (lo + 1.25, np.full(130, 2.5)), t=(250.0, 1.0, 0.8))
    add("ends_inside", 5, regular_bins(990.0, 1070.0, 1.0))
    add("starts_inside", 6, regular_bins(1030.0, 1110.0, 1.0))
    add("fine_bins", 7, regular_bins(995.0, 1035.0, 0.1), wn_grid=np.linspace(1000.0, 1030.0, 1001), t=(120.0, 0.01, 3.0))
    add("lorentz", 8, regular_bins(990.0, 1110.0, 1.0), lid=LORENTZ, t=(220.0, 0.6, 1.2))
    # Gaussian: alpha_d ~ 1e-3 cm-1 here, so bins of two Doppler widths -- the shape three bins away is ~1e-11 of the centre's
    add("gaussian", 9, regular_bins(999.95, 1000.25, 0.002), lid=GAUSSIAN, wn_grid=np.linspace(1000.0, 1000.2, 1001),
        t=(200.0, 0.1, 1.4))
    add("one_neighbour", 10, regular_bins(990.0, 1110.0, 1.0), nb=1)
    add("onto_nonzero", 11, regular_bins(990.0, 1110.0, 1.0), out0=10.0 ** np.random.default_rng(12).uniform(-27, -23, 1001))
    add("two_broadeners", 13, regular_bins(990.0, 1110.0, 1.0), M=2, t=(160.0, 0.2, 2.0))
    add("three_broadeners", 14, regular_bins(990.0, 1110.0, 2.0), M=3, t=(300.0, 2.0, 0.6))
    return cases


def load_golden(path):
    """name -> dict of the inputs and of the reference's out, store, store_x"""
    z = np.load(path)
    cases = {}
    for key in z.files:
        name, field = key.split("__", 1)
        v = z[key]
        cases.setdefault(name, {})[field] = v if v.ndim else v.item()
    return cases


def big_case(nw=200000, N=2000, L=4, seed=21):
    """2e5 grid points x 2000 bins x 4 layers, two broadeners: 1 cm-1 bins that start 100 cm-1 below the grid and end 100 cm-1
    before its end, so the last 10^4 grid points lie outside the bins"""
    rng = np.random.default_rng(seed)
    wn_grid = 2000.0 + 0.01 * np.arange(nw)                       # 2000 .. 4000
    centers, widths = regular_bins(1900.0, 1900.0 + N * 1.0, 1.0)  # 1900 .. 3900
    d = synth_bins(rng, centers, widths, 2)
    d.update(wn_grid=wn_grid, t_calc=np.linspace(120.0, 300.0, L), t_ref=296.0, p_calc=np.logspace(-3, 0, L), p_ref=1.0,
             q_ratio=np.linspace(2.5, 0.9, L), isotopic_abundance=0.75, isotopic_mass=44.0, lineshape_id=VOIGT,
             n_neighbour_bins=3)
    return d


def engine_args(d, L_index=None):
    """positional arguments of AnsfmEngine.add_pseudo_continuum_monochromatic_absorption up to lsw_mean_e_lower"""
    pick = (lambda a: a) if L_index is None else (lambda a: np.atleast_1d(a)[L_index])
    return (d["wn_grid"], int(d["lineshape_id"]), pick(d["t_calc"]), d["t_ref"], pick(d["p_calc"]), d["p_ref"], pick(d["q_ratio"]),
            d["isotopic_abundance"], d["isotopic_mass"], d["mol_mix_frac"], d["bparams"], d["centers"], d["widths"], d["sw_sum"],
            d["e_lower"])
