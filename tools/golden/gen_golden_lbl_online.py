"""Runtime line-by-line golden: the REFERENCE's Spectroscopy_0.calc_klbl_online (:2046) / calc_klblg_online (:1922) and the
ILBL = 1 branch of ForwardModel_0.calculate_gaseous_line_opacity (:3819-3848) on the seeded synthetic line data of
tests/lbl_online_cases.py.  No line database: a LineData_0 is built without its __init__ (object.__new__ and the private
fields that __init__ sets), its line_data / continuum_data come from LineSetSpecData.create_from / PseudoContSpecData.create_from
on namespaces of seeded arrays, its partition functions are analytic callables; Spectroscopy, Layer, Atmosphere and Scatter are
namespaces with the attributes the two routines read.

Per case: the line source after the host-side selections (LineSource.from_spectroscopy), the layers, amb_frac, the q ratios,
k, dkdT (the seam case also calc_klbl_online's k, whose sum order differs) and, through the forward-model branch with
gradients, TAUGAS and dTAUGAS.  Needs the reference (build container only).

    python tools/golden/gen_golden_lbl_online.py      # -> tests/golden/lbl_online.npz
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.ref_import import import_reference  # noqa: E402
import lbl_online_cases as oc  # noqa: E402
from archnemesis_dist_amd import line_source as lsrc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lbl_online.npz")
NS = types.SimpleNamespace


def make_line_data(ld, gas, mol_id, iso, amb, seed):
    """a LineData_0 without a database"""
    o = object.__new__(ld.LineData_0)
    o._ID, o._ISO = ld.INVALID_MOLECULE_ID, None
    o._ans_database = None
    o._rt_gas_descs = o._default_iso_abundances = o._n_isos = o._mol_ids = o._iso_ids = o._mol_id_tpl = o._iso_id_tpl = None
    o._params = ld.LineDataParams(ambient_gasses=amb)
    o._params_fetched_lines_last = o._params_fetched_partition_last = True
    o._combined_line_data = None
    o.ID, o.ISO, o.cache = mol_id, iso, None
    rng = (oc.WN_GRID[0] - 200.0, oc.WN_GRID[-1] + 200.0)
    o.line_data, o.continuum_data, o.partition_fn_data = [], [], []
    for i, desc in enumerate(o.rt_gas_descs):
        d = oc.raw_isotopologue(gas, i, len(amb), seed)
        lines = NS(s_min=1e-30, t_ref=oc.T_REF, p_ref=oc.P_REF, req_wn_range=rng, nu=d["nu"], sw=d["sw"], a=d["a"], elower=d["elower"],
                   gamma_self=d["gamma_self"], n_self=d["n_self"], gamma_amb=d["gamma_amb"], n_amb=d["n_amb"], delta_amb=d["delta_amb"])
        cont = NS(s_max=1e-30, t_cont=oc.T_REF, p_cont=oc.P_REF, req_wn_range=rng, wn_bin_center=d["wn_bin_center"],
                  wn_bin_width=d["wn_bin_width"], line_strength_sum=d["line_strength_sum"],
                  line_strength_weighted_mean_lower_energy_state=d["lsw_elower"], line_strength_weighted_gamma_self=d["lsw_gamma_self"],
                  line_strength_weighted_n_self=d["lsw_n_self"], line_strength_weighted_gamma_amb=d["lsw_gamma_amb"],
                  line_strength_weighted_n_amb=d["lsw_n_amb"])
        o.line_data.append(ld.LineSetSpecData.create_from(desc.gas_id, desc.iso_id, amb, lines))
        o.continuum_data.append(ld.PseudoContSpecData.create_from(desc.gas_id, desc.iso_id, amb, cont))
        o.partition_fn_data.append(oc.PowerQ(*oc.q_params(gas, i)))
    assert len(o.line_data) == oc.GASES[gas][2], (mol_id, iso, len(o.line_data))
    return o


def main():
    import_reference()
    ans = importlib.import_module("archnemesis")
    ld = importlib.import_module("archnemesis.LineData_0")
    sp = importlib.import_module("archnemesis.Spectroscopy_0")
    fm = importlib.import_module("archnemesis.ForwardModel_0")
    E = ans.enum
    amb_all = (E.AmbientGasEnum.AIR, E.AmbientGasEnum.CO2)
    # every line-shape value that enters a sum is watched: no expected value rests on subnormal arithmetic
    smallest = [np.inf]
    to_fn = sp.SpectroscopicLineProfileEnum_to_lineshape_fn

    def watched_fn(shape):
        f = to_fn(shape)

        def watched(dwn, alpha_d, gamma_l):
            v = f(dwn, alpha_d, gamma_l)
            if v != 0.0:
                smallest[0] = min(smallest[0], float(v))
            return v
        return watched
    sp.SpectroscopicLineProfileEnum_to_lineshape_fn = watched_fn

    blob = {}
    for name, c in oc.CASES.items():
        amb = amb_all[: c["n_amb"]]
        S = NS(WAVE=oc.WN_GRID.copy(), NWAVE=oc.WN_GRID.size, NG=1, NGAS=len(oc.GASES), ID=[g[0] for g in oc.GASES],
               ISO=[g[1] for g in oc.GASES], ISPACE=E.WaveUnitEnum.Wavenumber_cm, N_AMB_GASSES=len(amb),
               ILBL=E.SpectralCalculationModeEnum.LINE_BY_LINE_RUNTIME)
        S.LINE_DATA = [make_line_data(ld, s, g[0], g[1], amb, c["seed"]) for s, g in enumerate(oc.GASES)]
        S.LINE_DATA_PARAMS = [sp.MolLineDataParams(lineshape=E.SpectroscopicLineProfileEnum(c["lineshape"]), amb_gas=amb, s_min=-1.0,
                                                   s_floor=0.0, use_cache=False)._replace(**p) for p in c["params"]]
        S.calc_klbl_online = types.MethodType(sp.Spectroscopy_0.calc_klbl_online, S)
        S.calc_klblg_online = types.MethodType(sp.Spectroscopy_0.calc_klblg_online, S)
        lay = oc.layers(name)
        L = c["nlay"]
        press_atm = lay["PRESS"] / fm.ATM_TO_PASCAL
        pre = name + "__"
        smallest[0] = np.inf
        if c["kind"] == "fm":
            A = NS(NVMR=3, ID=lay["ATM_ID"], ISO=lay["ATM_ISO"])
            A.locate_gas = lambda gid, iso, A=A: int(np.flatnonzero((A.ID == gid) & (A.ISO == iso))[0])
            F = NS(SpectroscopyX=S, AtmosphereX=A, ScatterX=NS(NDUST=0),
                   LayerX=NS(NLAY=L, PRESS=lay["PRESS"], TEMP=lay["TEMP"], PP=lay["PP"], AMOUNT=lay["AMOUNT"]))
            TAUGAS, dTAUGAS = fm.ForwardModel_0.calculate_gaseous_line_opacity(F, return_grad=True)
            amb_frac = lsrc.ambient_fractions(lay["PP"], lay["PRESS"], lay["ATM_ID"], S.ID)
            blob[pre + "TAUGAS"], blob[pre + "dTAUGAS"] = TAUGAS, dTAUGAS
            blob[pre + "igas"] = np.array([A.locate_gas(i, j) for i, j in zip(S.ID, S.ISO)])
        else:
            amb_frac = c["amb_frac"]
        k_f = S.calc_klbl_online(L, press_atm, lay["TEMP"], amb_frac=amb_frac)
        k, dkdT = S.calc_klblg_online(L, press_atm, lay["TEMP"], amb_frac=amb_frac)
        assert smallest[0] >= 1e-280, (name, smallest[0])
        nz = k[k != 0.0]
        assert np.all(k >= 0) and nz.size > 0.99 * k.size and nz.min() > 1e-280, (name, nz.min())
        rel = np.max(np.abs(k_f - k) / k.max())
        source = lsrc.LineSource.from_spectroscopy(S)
        assert source.unsupported() is None, source.unsupported()
        oc.source_to_blob(source, pre + "src_", blob)
        n_sel = [[(iso.N, iso.Nb) for iso in g] for g in source.gases]
        mix = lsrc.mix_fractions(np.broadcast_to(amb_frac, (len(oc.GASES), len(amb))))
        st = lsrc.pack_line_state(source, press_atm, lay["TEMP"], mix, grad=True)
        for key in ("PRESS", "TEMP", "PP", "AMOUNT", "ATM_ID", "ATM_ISO"):
            blob[pre + key] = lay[key]
        blob[pre + "amb_frac"], blob[pre + "mix"] = np.asarray(amb_frac, dtype=float), mix
        # the q ratios with the reference's expression (LineData_0.py:848, :1374), per (gas, isotopologue, layer)
        for tag, dT in (("", 0.0), ("_dT", 5.0)):
            for s, ldo in enumerate(S.LINE_DATA):
                blob[f"{pre}q_lines{tag}_g{s}"] = np.array([[pf(ls.t_ref) / pf(t + dT) for t in lay["TEMP"]]
                                                            for pf, ls in zip(ldo.partition_fn_data, ldo.line_data)])
                blob[f"{pre}q_cont{tag}_g{s}"] = np.array([[pf(pc.t_cont) / pf(t + dT) for t in lay["TEMP"]]
                                                           for pf, pc in zip(ldo.partition_fn_data, ldo.continuum_data)])
        blob[pre + "k"], blob[pre + "dkdT"] = k, dkdT
        if c["kind"] == "seam":                 # calc_klbl_online's own sum order: (sum lines) + (sum continuum)
            blob[pre + "k_fwd"] = k_f
        print(f"{name:12s} L={L} M={len(amb) + 1} (lines, bins) after the masks {n_sel}  rows {st.R}  smallest shape {smallest[0]:.2e}  "
              f"k in [{nz.min():.2e}, {k.max():.2e}]  forward vs gradient seam {rel:.1e}")
        # the masks bite: lines and bins were dropped
        assert any(iso.Nb < oc.raw_isotopologue(s, i, len(amb), c["seed"])["wn_bin_center"].size for s, g in enumerate(source.gases)
                   for i, iso in enumerate(g))
        assert any(iso.N < oc.raw_isotopologue(s, i, len(amb), c["seed"])["nu"].size for s, g in enumerate(source.gases)
                   for i, iso in enumerate(g))
    np.savez_compressed(OUT, **blob)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 600_000


if __name__ == "__main__":
    main()
