"""Seeded synthetic atmospheres / k-tables for bench.py and the parity tests.

No model keys, no real data: the reference's own k-tables are not redistributable blobs, so the
benchmark configuration is defined by these generators.  NumPy only (host); bench.py moves the
arrays to HBM before timing.
"""
import numpy as np


def gauss_legendre_01(ng, as_float32=False):
    """g-ordinates / weights on [0,1] (Gauss-Legendre), optionally rounded to float32 like a
    .kta header (Spectroscopy_0.py:2951-3031)."""
    x, w = np.polynomial.legendre.leggauss(ng)
    g_ord = 0.5 * (x + 1.0)
    del_g = 0.5 * w
    if as_float32:
        g_ord = g_ord.astype(np.float32).astype(np.float64)
        del_g = del_g.astype(np.float32).astype(np.float64)
    return g_ord, del_g


def synth_ktable(W, G, NP, NT, S, seed=20260704, zero_low_g=False, chunk=512, out=None):
    """K (W,G,NP,NT,S): log-uniform 1e-30..1e-18 cm^2, non-decreasing in g, smooth in (p,T).
    PRESS logspace(-7,1.3) atm, TEMP linspace(50,500) K."""
    rng = np.random.default_rng(seed)
    PRESS = np.logspace(-7, 1.3, NP)
    TEMP = np.linspace(50.0, 500.0, NT)
    K = np.empty((W, G, NP, NT, S)) if out is None else out
    for w0 in range(0, W, chunk):
        w1 = min(W, w0 + chunk)
        n = w1 - w0
        base = 10.0 ** rng.uniform(-28, -21, size=(n, 1, 1, 1, S))
        gshape = np.sort(10.0 ** rng.uniform(-2, 3, size=(n, G, 1, 1, S)), axis=1)
        pexp = rng.uniform(0.0, 0.3, size=(n, 1, 1, 1, S))
        texp = rng.uniform(-1.0, 2.0, size=(n, 1, 1, 1, S))
        blk = base * gshape * PRESS[None, None, :, None, None] ** pexp * (TEMP[None, None, None, :, None] / 200.0) ** texp
        if zero_low_g:
            ncut = rng.integers(0, 4, size=(n, 1, NP, NT, S))
            blk = np.where(np.arange(G)[None, :, None, None, None] < ncut, 0.0, blk)
        K[w0:w1] = blk
    return PRESS, TEMP, K


def synth_atmosphere(L, S, seed=7, n_models=1, perturb=0.0):
    """Nadir atmosphere, L equal-log-p layers 10 bar -> 1e-6 bar (bottom -> top, like Layer_0).
    Returns dict of per-model arrays: lay_press_pa (n,L), lay_temp (n,L), amount (n,S,L) in cm^-2."""
    rng = np.random.default_rng(seed)
    p_bar = np.logspace(1, -6, L)
    press_pa = p_bar * 1e5
    z = np.linspace(0, 1, L)
    temp = 110.0 + 290.0 * (1.0 - z) ** 3 + 60.0 * z ** 2        # 110..400 K analytic profile
    vmr = 10.0 ** rng.uniform(-9, -1, size=S)
    # column density of a layer ~ dp/(g*mu): molecules cm^-2
    dlnp = np.log(p_bar[0] / p_bar[1])
    totam = press_pa * dlnp / (24.8 * 2.3 * 1.6605e-27) * 1e-4
    amount = vmr[:, None] * totam[None, :]
    lp = np.repeat(press_pa[None], n_models, 0)
    lt = np.repeat(temp[None], n_models, 0)
    am = np.repeat(amount[None], n_models, 0)
    if perturb and n_models > 1:
        # model 0 = base state; model i>0 perturbs one element by +5 % (jacobian_nemesis :2234-2242):
        # first L perturbations: T of layer i-1; next L: amount of gas 0 in layer i-1-L; then cycle
        for i in range(1, n_models):
            j = (i - 1) % (2 * L)
            if j < L:
                lt[i, j] *= (1.0 + perturb)
            else:
                am[i, 0, j - L] *= (1.0 + perturb)
    return dict(lay_press_pa=lp, lay_temp=lt, amount=am)


def nadir_path(L, emiss_ang=0.0):
    """PathX for a nadir ray: layers used top -> bottom (AtmCalc_0.py:355-375), SCALE = 1/cos(emi)."""
    LAYINC = np.arange(L - 1, -1, -1, dtype=np.int32)[:, None]
    NLAYIN = np.array([L], dtype=np.int32)
    SCALE = np.full((L, 1), 1.0 / np.cos(np.deg2rad(emiss_ang)))
    return NLAYIN, LAYINC, SCALE


def synth_continuum(W, L, seed=3, n_models=1):
    """Smooth seeded (W,L) continuum opacity standing in for TAUCIA+TAUDUST+TAURAY."""
    rng = np.random.default_rng(seed)
    wv = np.linspace(0, 1, W)[:, None]
    lv = np.linspace(0, 1, L)[None, :]
    base = 1e-3 * np.exp(-6.0 * lv) * (1.0 + 0.5 * np.sin(9.0 * wv + rng.uniform(0, 6.28)))
    return np.repeat(base[None], n_models, 0)


# Jovian-like composition of the synthetic profile set: H2 and He carry the bulk (and the Rayleigh opacity, IRAY = 4),
# the k-table gases are CH4, NH3 and trace species.  IDs are the radtran gas numbers the reference uses.
PROFILE_GAS_ID = np.array([39, 40, 6, 11, 26, 27, 28, 32, 33, 41, 1, 2, 4, 5, 7, 8, 9, 10, 12, 13, 14, 15], dtype=np.int32)


def synth_profiles(NPRO, NVMR, seed=11, p_bottom_bar=10.0, p_top_bar=1.0e-6):
    """Reference-atmosphere profiles on NPRO levels (bottom -> top, like Atmosphere_0): H (m) from the hydrostatic
    equation of an H2/He atmosphere (g = 24.8 m s-2), P (Pa), T (K) 110..400 K, VMR (NPRO, NVMR) with H2, He first and
    NVMR - 2 absorbers (log-uniform 1e-9 .. 1e-3, mild vertical gradient).  Returns dict(H, P, T, VMR, ID, ISO, RADIUS)."""
    if not 3 <= NVMR <= PROFILE_GAS_ID.size:
        raise ValueError("synth_profiles: 3 <= NVMR <= %d" % PROFILE_GAS_ID.size)
    rng = np.random.default_rng(seed)
    p_bar = np.logspace(np.log10(p_bottom_bar), np.log10(p_top_bar), NPRO)
    z = np.linspace(0.0, 1.0, NPRO)
    T = 110.0 + 290.0 * (1.0 - z) ** 3 + 60.0 * z ** 2
    scale_height = 8.314462618 * T / (2.3e-3 * 24.8)                       # R T / (mu g), m
    dlnp = -np.diff(np.log(p_bar))
    H = np.concatenate([[0.0], np.cumsum(0.5 * (scale_height[1:] + scale_height[:-1]) * dlnp)])
    VMR = np.empty((NPRO, NVMR))
    trace = 10.0 ** rng.uniform(-9, -3, NVMR - 2)
    slope = rng.uniform(-0.5, 0.5, NVMR - 2)
    VMR[:, 2:] = trace[None, :] * (p_bar[:, None] / p_bar[0]) ** (0.1 * slope[None, :])
    rest = 1.0 - VMR[:, 2:].sum(axis=1)
    VMR[:, 0] = 0.864 * rest
    VMR[:, 1] = 0.136 * rest
    return dict(H=H, P=p_bar * 1.0e5, T=T, VMR=VMR, ID=PROFILE_GAS_ID[:NVMR].copy(), ISO=np.zeros(NVMR, dtype=np.int32),
                RADIUS=7.1492e7)


def synth_cia(NWC=400, NT=10, wn_max=2000.0, seed=13):
    """Collision-induced absorption table of an H2 / He atmosphere (pairs H2-H2 and H2-He, no ortho/para axis): smooth bands
    of 1e-46 .. 1e-44 cm^5 molecule^-2 on NWC wavenumbers 0 .. wn_max and NT temperatures 50 .. 500 K, growing with
    temperature.  Returns the dict `BatchedCKThermalModel(cia=...)` and, by name, `AnsfmEngine.upload_cia` take."""
    rng = np.random.default_rng(seed)
    wn = np.linspace(0.0, wn_max, NWC)
    temp = np.linspace(50.0, 500.0, NT)
    K = np.empty((2, 1, NT, NWC))
    for ip in range(2):
        centre, width = rng.uniform(300.0, 900.0, 3), rng.uniform(150.0, 400.0, 3)
        band = sum(np.exp(-0.5 * ((wn - c) / w) ** 2) for c, w in zip(centre, width))
        K[ip, 0] = 10.0 ** rng.uniform(-46, -45) * (1.0 + 9.0 * band[None, :]) * (temp[:, None] / 100.0) ** rng.uniform(0.3, 0.9)
    return dict(CIA_WAVEN=wn, CIA_TEMP=temp, CIA_FRAC=np.array([0.0]), NPARA=0, K_CIA=K, IPAIRG1=[39, 39], IPAIRG2=[39, 40],
                INORMALT=[0, 0], INORMAL=0, INORMALD=np.array([False, False]))


def synth_lbl_gas(wn_lo, wn_hi, n_iso, lines, L, seed=0, bin_width=1.0, margin=150.0):
    """Runtime line-by-line data of a synthetic gas of n_iso isotopologues between wn_lo and wn_hi (cm-1): per isotopologue
    `lines` strong lines and the weak-line bins of width bin_width, both out to `margin` beyond the interval, one broadener.
    Returns a list of (line_args, continuum_args): the arguments of AnsfmEngine.add_line_set_monochromatic_absorption from
    t_ref on without p_calc (lineshape_id first) and of add_pseudo_continuum_monochromatic_absorption likewise -- what
    LblAccumulator.add_lines / add_pseudo_continuum take."""
    rng = np.random.default_rng(seed)
    c2 = 2.99792458E10 * 6.62607015E-27 / 1.380649E-16
    t_ref, p_ref, mmf = 296.0, 1.0, np.array([1.0])
    nbin = int(round((wn_hi - wn_lo + 2 * margin) / bin_width))
    centers = wn_lo - margin + bin_width * (np.arange(nbin) + 0.5)
    widths = np.full(nbin, float(bin_width))

    def broadening(n):
        bp = np.zeros((3, n))
        bp[0] = rng.uniform(0.02, 0.1, n); bp[1] = rng.uniform(0.5, 0.8, n); bp[2] = rng.uniform(-0.01, 0.01, n)
        return bp

    out = []
    for iso in range(n_iso):
        abundance, mass = (0.98, 0.011, 0.004, 0.002)[iso % 4], 28.0 + iso
        q = np.linspace(1.8, 1.0, L) * (1.0 + 0.05 * iso)
        nu = np.sort(rng.uniform(wn_lo - 75.0, wn_hi + 75.0, lines))
        line_args = (0, t_ref, p_ref, q, abundance, mass, mmf, broadening(lines), nu, 10.0 ** rng.uniform(-28, -19, lines),
                     rng.uniform(0, 3000, lines), 1 - np.exp(-c2 * nu / t_ref))
        cont_args = (0, t_ref, p_ref, q, abundance, mass, mmf, broadening(nbin), centers, widths,
                     10.0 ** rng.uniform(-27, -23, nbin), rng.uniform(0, 3000, nbin))
        out.append((line_args, cont_args))
    return out


class PowerLawQ:
    """partition function Q(T) = a T^b, the stand-in of the synthetic line sources"""

    def __init__(self, a, b):
        self.a, self.b = float(a), float(b)

    def __call__(self, t):
        return self.a * t ** self.b


def synth_line_source(wn_grid, n_iso=(3,), lines=1000, seed=0, bin_width=1.0, margin=150.0):
    """A `line_source.LineSource` of synthetic gases on wn_grid (ascending cm-1): n_iso[s] isotopologues of gas s, each with
    `lines` Voigt lines and the weak-line bins of width bin_width out to `margin` beyond the grid, broadened by "self" and one
    ambient gas (M = 2), partition functions Q = a T^b."""
    from .line_source import Isotopologue, LineSource
    rng = np.random.default_rng(seed)
    c2 = 2.99792458E10 * 6.62607015E-27 / 1.380649E-16
    lo, hi = float(wn_grid[0]), float(wn_grid[-1])
    nbin = int(round((hi - lo + 2 * margin) / bin_width))
    centers = lo - margin + bin_width * (np.arange(nbin) + 0.5)

    def broadening(n):
        bp = np.zeros((6, n))
        bp[0] = rng.uniform(0.05, 0.12, n); bp[1] = rng.uniform(0.5, 0.8, n)                                     # self: no shift
        bp[3] = rng.uniform(0.02, 0.1, n); bp[4] = rng.uniform(0.5, 0.8, n); bp[5] = rng.uniform(-0.01, 0.01, n)
        return bp

    gases = []
    for s, n in enumerate(n_iso):
        isos = []
        for i in range(n):
            nu = np.sort(rng.uniform(lo - 75.0, hi + 75.0, lines))
            pcb = broadening(nbin); pcb[5] = 0.0
            isos.append(Isotopologue(0, (0.98, 0.011, 0.004, 0.002)[i % 4], 28.0 + i + 4 * s, PowerLawQ(2.0 + i, 1.5 + 0.1 * s), 2,
                                     bparams=broadening(lines), nu=nu, sw=10.0 ** rng.uniform(-28, -19, lines),
                                     e_lower=rng.uniform(0, 3000, lines), stim_ref=1 - np.exp(-c2 * nu / 296.0), pc_bparams=pcb,
                                     centers=centers, widths=np.full(nbin, float(bin_width)), sw_sum=10.0 ** rng.uniform(-27, -23, nbin),
                                     pc_e_lower=rng.uniform(0, 3000, nbin)))
        gases.append(isos)
    return LineSource(wn_grid, gases, 2)
