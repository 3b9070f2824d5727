"""Seeded synthetic line data of the runtime line-by-line fixture (tests/golden/lbl_online.npz), shared by the generator
(tools/golden/gen_golden_lbl_online.py, which feeds them to the reference) and the tests, which read the recorded arrays.

Two gases, as the reference names them: ID 6 / ISO 0 (four isotopologues, the third without lines) and ID 5 / ISO 1 (one).
801 grid points (no multiple of 64), <= 120 lines per isotopologue, lines and bins beyond the wn_calc_range so the masks of
LineData_0.add_monochromatic_absorption bite.  Partition functions are the analytic Q(T) = a T^b.
"""
import numpy as np

VOIGT, LORENTZ = 0, 4
WN_GRID = 1000.0 + 0.05 * np.arange(801)
GASES = ((6, 0, 4), (5, 1, 1))              # (ID, ISO, isotopologues)
T_REF, P_REF = 296.0, 1.0


class PowerQ:
    """Q(T) = a T^b"""

    def __init__(self, a, b):
        self.a, self.b = float(a), float(b)

    def __call__(self, t):
        return self.a * t ** self.b


def q_params(gas, iso):
    return 3.0 + gas + 0.5 * iso, 1.5 + 0.1 * iso + 0.05 * gas


def raw_isotopologue(gas, iso, n_amb, seed, n_lines=None):
    """what LineSetData / PseudoContinuumData hold for one isotopologue, before any selection"""
    r = np.random.default_rng(1000 * seed + 10 * gas + iso)
    N = (0 if (gas == 0 and iso == 2) else 60 + 20 * ((gas + iso) % 4)) if n_lines is None else n_lines
    # lines from 180 cm-1 below the grid to 180 above: the range of the masks ends 150 cm-1 (2 x 75) outside it
    nu = r.uniform(WN_GRID[0] - 180.0, WN_GRID[-1] + 180.0, N)
    nu[: N // 2] = r.uniform(WN_GRID[0] - 5.0, WN_GRID[-1] + 5.0, N // 2)
    d = dict(nu=nu, sw=10.0 ** r.uniform(-23.0, -19.5, N), a=r.uniform(0.1, 10.0, N), elower=r.uniform(10.0, 1500.0, N),
             gamma_self=r.uniform(0.05, 0.12, N), n_self=r.uniform(0.5, 0.8, N), gamma_amb=r.uniform(0.03, 0.09, (N, n_amb)),
             n_amb=r.uniform(0.55, 0.8, (N, n_amb)), delta_amb=r.uniform(-0.01, 0.004, (N, n_amb)))
    # bins 4 cm-1 wide from 162 below the grid to 162 above; every fifth one empty
    c = np.arange(WN_GRID[0] - 162.0, WN_GRID[-1] + 162.0, 4.0) + 0.37
    Nb = c.size
    sw_sum = 10.0 ** r.uniform(-24.0, -22.0, Nb)
    sw_sum[::5] = 0.0
    d.update(wn_bin_center=c, wn_bin_width=np.full(Nb, 4.0), line_strength_sum=sw_sum,
             lsw_elower=r.uniform(50.0, 900.0, Nb), lsw_gamma_self=r.uniform(0.05, 0.1, Nb), lsw_n_self=r.uniform(0.5, 0.8, Nb),
             lsw_gamma_amb=r.uniform(0.03, 0.08, (Nb, n_amb)), lsw_n_amb=r.uniform(0.55, 0.8, (Nb, n_amb)))
    return d


# name -> what the generator sets up.  params per gas: the fields of MolLineDataParams that differ from their defaults
# (25 / 75 cm-1 windows, s_floor 0, everything included).  "fm": through calculate_gaseous_line_opacity (one ambient gas:
# amb_frac comes out (NGAS, 1)); "seam": calc_klbl_online / calc_klblg_online with amb_frac (NGAS, n_amb).
CASES = {
    "voigt_fm": dict(kind="fm", seed=1, n_amb=1, lineshape=VOIGT, nlay=4,
                     params=[dict(), dict(s_floor=3.0e-22)]),
    "lorentz_fm": dict(kind="fm", seed=2, n_amb=1, lineshape=LORENTZ, nlay=2,
                       params=[dict(include_pressure_shift=False), dict(include_continuum=False)]),
    "voigt_seam3": dict(kind="seam", seed=3, n_amb=2, lineshape=VOIGT, nlay=2,
                        params=[dict(), dict()], amb_frac=np.array([[0.55, 0.3], [0.7, 0.25]])),
}


def layers(case):
    """the layer quantities the ILBL = 1 branch reads: PRESS (Pa), TEMP, PP (NLAY, NVMR) (Pa), AMOUNT (NLAY, NVMR) (cm-2) for
    an atmosphere of three gases: ID 6 / ISO 0, ID 5 / ISO 1 and a filler (ID 22 / ISO 0)"""
    c = CASES[case]
    r = np.random.default_rng(77 + c["seed"])
    L = c["nlay"]
    press = 101325.0 * np.geomspace(0.8, 0.02, L)
    temp = np.linspace(285.0, 215.0, L) + r.uniform(-2.0, 2.0, L)
    vmr = np.stack([np.full(L, 0.04) * r.uniform(0.9, 1.1, L), np.full(L, 0.02) * r.uniform(0.9, 1.1, L), np.full(L, 0.9)], axis=1)
    amount = vmr * (press / temp)[:, None] * 5.0e21
    return dict(PRESS=press, TEMP=temp, PP=vmr * press[:, None], AMOUNT=amount, ATM_ID=np.array([6, 5, 22]),
                ATM_ISO=np.array([0, 1, 0]))


# ---- the fixture ------------------------------------------------------------------------------------------------------------
ISO_SCALARS = ("lineshape_id", "abundance", "mass", "t_ref", "p_ref", "s_floor", "wn_calc_window", "wn_approx_window",
               "include_lines", "t_cont", "p_cont", "n_neighbour_bins", "include_continuum")
ISO_ARRAYS = ("bparams", "nu", "sw", "e_lower", "stim_ref", "pc_bparams", "centers", "widths", "sw_sum", "pc_e_lower")


def source_to_blob(source, prefix, blob):
    """a LineSource (after the host-side selections) as arrays"""
    blob[prefix + "wn_grid"] = source.wn_grid
    blob[prefix + "M"] = np.array(source.M)
    blob[prefix + "n_iso"] = np.array(source.n_iso)
    for s, isos in enumerate(source.gases):
        for i, iso in enumerate(isos):
            blob[f"{prefix}g{s}i{i}_scalars"] = np.array([float(x) for x in iso.scalars()])
            blob[f"{prefix}g{s}i{i}_q"] = np.array(q_params(s, i))
            for name, a in zip(ISO_ARRAYS, iso.arrays()):
                blob[f"{prefix}g{s}i{i}_{name}"] = a


def source_from_blob(z, prefix):
    from archnemesis_dist_amd.line_source import Isotopologue, LineSource
    M = int(z[prefix + "M"])
    gases = []
    for s, n in enumerate(z[prefix + "n_iso"]):
        isos = []
        for i in range(int(n)):
            sc = dict(zip(ISO_SCALARS, z[f"{prefix}g{s}i{i}_scalars"]))
            arr = {name: z[f"{prefix}g{s}i{i}_{name}"] for name in ISO_ARRAYS}
            isos.append(Isotopologue(int(sc["lineshape_id"]), sc["abundance"], sc["mass"], PowerQ(*z[f"{prefix}g{s}i{i}_q"]), M,
                                     t_ref=sc["t_ref"], p_ref=sc["p_ref"], s_floor=sc["s_floor"], wn_calc_window=sc["wn_calc_window"],
                                     wn_approx_window=sc["wn_approx_window"], include_lines=bool(sc["include_lines"]),
                                     t_cont=sc["t_cont"], p_cont=sc["p_cont"], n_neighbour_bins=int(sc["n_neighbour_bins"]),
                                     include_continuum=bool(sc["include_continuum"]), **arr))
        gases.append(isos)
    return LineSource(z[prefix + "wn_grid"], gases, M)
