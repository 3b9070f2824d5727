"""The host side of CIRSrad on runtime line-by-line opacities (ILBL = 1), without a GPU: the packer of the distinct k-rows,
the line source read from LINE_DATA-like objects, and the CIRSradGPU adapter driven with a recording engine double --
supported and delegated cases, amb_frac and the q ratios against the reference's (tests/golden/lbl_online.npz).  The error
codes of the C entries need a context and are in tests/test_lbl_online_gpu.py."""
import os
import types

import numpy as np
import pytest

import lbl_online_cases as oc
from archnemesis_dist_amd import forward_model as fm
from archnemesis_dist_amd import line_source as ls

NS = types.SimpleNamespace
ATM = 101325.0


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "lbl_online.npz"))
    return {k: z[k] for k in z.files}


def _g(golden, name, key):
    return golden[f"{name}__{key}"]


# ---- the packer -----------------------------------------------------------------------------------------------------------------
def test_packer_finds_the_distinct_rows_by_bits(golden):
    name = "voigt_fm"
    src = oc.source_from_blob(golden, name + "__src_")
    p, t, mix = _g(golden, name, "PRESS") / ATM, _g(golden, name, "TEMP"), _g(golden, name, "mix")
    L, S = p.size, src.S
    st = ls.pack_line_state(src, p, t, mix, grad=True)
    assert (st.n, st.S, st.L, st.R) == (1, S, L, S * L) and st.krow.dtype == np.int32 and st.row_gas.dtype == np.int32
    assert np.array_equal(st.krow[0], np.arange(S * L).reshape(S, L)) and np.array_equal(st.row_gas, np.repeat(np.arange(S), L))
    assert np.array_equal(st.row_p_atm, np.tile(p, S)) and np.array_equal(st.row_mix, np.repeat(mix, L, axis=0))
    # four states: state 0, a layer temperature, gas 0's mix fractions, a copy of state 0 -- and a -0.0 that is not 0.0
    P, T, MIX = np.repeat(p[None], 5, 0), np.repeat(t[None], 5, 0), np.repeat(mix[None], 5, 0)
    T[1, 2] += 1.5
    MIX[2, 0] = [0.9, 0.1]
    P[4, 1] = np.nextafter(P[4, 1], 1.0)                                     # one bit
    st = ls.pack_line_state(src, P, T, MIX)
    assert st.R == S * L + S + L + S and not st.grad
    assert np.array_equal(st.krow[3], st.krow[0]) and np.all(np.diff(st.row_gas) >= 0)
    for m in range(5):                                                       # every (model, gas, layer) finds its own numbers
        for s in range(S):
            r = st.krow[m, s]
            assert np.array_equal(st.row_gas[r], np.full(L, s))
            assert np.array_equal(st.row_p_atm[r].view(np.uint64), P[m].view(np.uint64))
            assert np.array_equal(st.row_t[r], T[m]) and np.array_equal(st.row_mix[r], np.repeat(MIX[m, s][None], L, 0))
    changed = st.krow != st.krow[0]
    assert changed[1].sum() == S and changed[2].sum() == L and changed[2, 0].all() and changed[4].sum() == S
    # rows of different layers that hold the same numbers are one row
    st2 = ls.pack_line_state(src, np.full(3, 0.5), np.full(3, 250.0), mix)
    assert st2.R == S and np.array_equal(st2.krow[0], np.repeat(np.arange(S)[:, None], 3, 1))


def test_q_ratios_and_mix_fractions_against_the_reference(golden):
    for name, c in oc.CASES.items():
        src = oc.source_from_blob(golden, name + "__src_")
        p, t = _g(golden, name, "PRESS") / ATM, _g(golden, name, "TEMP")
        L = p.size
        assert np.array_equal(ls.mix_fractions(np.broadcast_to(_g(golden, name, "amb_frac"), (src.S, src.M - 1))), _g(golden, name, "mix"))
        st = ls.pack_line_state(src, p, t, _g(golden, name, "mix"), grad=True)
        o = 0
        for s, n_iso in enumerate(src.n_iso):                                # rows are grouped by gas: [L][n_iso] blocks
            for key, got in (("q_lines", st.row_q_lines), ("q_cont", st.row_q_cont), ("q_lines_dT", st.row_q_lines_dT),
                             ("q_cont_dT", st.row_q_cont_dT)):
                assert np.array_equal(got[o:o + L * n_iso].reshape(L, n_iso).T, _g(golden, name, f"{key}_g{s}")), (name, key, s)
            o += L * n_iso
        if c["kind"] == "fm":                                                # amb_frac of ForwardModel_0.py:3822-3827
            amb = ls.ambient_fractions(_g(golden, name, "PP"), _g(golden, name, "PRESS"), _g(golden, name, "ATM_ID"),
                                       [g[0] for g in oc.GASES])
            assert np.array_equal(amb, _g(golden, name, "amb_frac")) and amb.shape == (src.S, 1)


# ---- LINE_DATA-like objects, as LineSource.from_spectroscopy reads them ----------------------------------------------------
def _line_data_objects(src, wide=True):
    """stand-ins for LineData_0 built from a line source; wide: two extra lines and bins far outside the wn_calc_range, which
    the masks must drop again"""
    out = []
    far = np.array([src.wn_grid[0] - 400.0, src.wn_grid[-1] + 400.0])
    for s, isos in enumerate(src.gases):
        lines, conts = [], []
        for iso in isos:
            data = np.vstack([iso.nu, iso.sw, iso.e_lower, iso.stim_ref, np.zeros(iso.N), iso.bparams])
            if wide and iso.N:
                extra = np.repeat(data[:, :1], 2, 1); extra[0] = far
                data = np.hstack([extra[:, :1], data, extra[:, 1:]])
            lines.append(NS(_data=data, NU=data[0], has_data=data.shape[1] != 0, t_ref=iso.t_ref, p_ref=iso.p_ref,
                            _molecular_mass=iso.mass, broadening_molecule_ids=tuple(range(-1, src.M - 1))))
            cd = np.vstack([iso.centers, iso.widths, iso.sw_sum, iso.pc_e_lower, iso.pc_bparams])
            if wide:
                extra = np.repeat(cd[:, :1], 2, 1); extra[0] = far
                cd = np.hstack([extra[:, :1], cd, extra[:, 1:]])
            conts.append(NS(_data=cd, WN_BIN_CENTER=cd[0], WAVE_AND_LINE_DATA=cd[:4], ALL_BROADENING_LSW_PARAMS=cd[4:],
                            has_data=bool(np.any(cd[2] != 0)), t_cont=iso.t_cont, p_cont=iso.p_cont))
        out.append(NS(ISO=0 if len(isos) > 1 else 1, default_iso_abundances=np.array([i.abundance for i in isos]), line_data=lines,
                      continuum_data=conts, partition_fn_data=[i.partition_fn for i in isos]))
    return out


def _params(src, **over):
    out = []
    for isos in src.gases:
        i0 = isos[0]
        d = dict(lineshape=i0.lineshape_id, wn_calc_window=i0.wn_calc_window, wn_approx_window=i0.wn_approx_window, s_floor=i0.s_floor,
                 isotopic_abundance=None, include_pressure_shift=True, include_continuum=i0.include_continuum,
                 include_lines=i0.include_lines, use_cache=True)
        d.update(over)
        out.append(NS(**d))
    return out


def _model(golden, name, imod=fm.IMOD_THERMAL_EMISSION, **over):
    src = oc.source_from_blob(golden, name + "__src_")

    class Model(fm.CIRSradGPU):
        pass

    m = Model()
    L = _g(golden, name, "PRESS").size
    m.SpectroscopyX = NS(NGAS=src.S, ILBL=1, K=None, WAVE=src.wn_grid, NWAVE=src.nw, ISPACE=0, ID=[g[0] for g in oc.GASES],
                         ISO=[g[1] for g in oc.GASES], LINE_DATA=_line_data_objects(src), LINE_DATA_PARAMS=_params(src, **over))
    atm_id, atm_iso = _g(golden, name, "ATM_ID"), _g(golden, name, "ATM_ISO")
    m.AtmosphereX = NS(NVMR=3, ID=atm_id, ISO=atm_iso,
                       locate_gas=lambda gid, iso: int(np.flatnonzero((atm_id == gid) & (atm_iso == iso))[0]))
    m.ScatterX = NS(NDUST=0)
    from archnemesis_dist_amd import synthetic as syn
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, 10.0)
    lt = _g(golden, name, "TEMP")
    m.PathX = NS(IMOD=np.array([imod]), NPATH=1, NLAYIN=NLAYIN, LAYINC=LAYINC, SCALE=SCALE, EMTEMP=lt[LAYINC[:, 0]][:, None],
                 SOL_ANG=np.array([0.0]), EMISS_ANG=np.array([10.0]))
    m.LayerX = NS(NLAY=L, PRESS=_g(golden, name, "PRESS"), TEMP=lt, PP=_g(golden, name, "PP"), AMOUNT=_g(golden, name, "AMOUNT"))
    m.SurfaceX = NS(TSURF=-1.0)
    m.MeasurementX = NS(IFORM=0, ISPACE=0)
    return m, src


class RecordingEngine:
    """what the adapter asks of the engine, recorded; results are zeros of the right shape"""

    def __init__(self):
        self.calls = []

    def upload_line_source(self, source):
        self.calls.append(("upload_line_source", source))
        self.dims = (source.nw, 1, 2, 2, source.S)

    def set_line_state(self, state):
        self.calls.append(("set_line_state", state))

    def cirsrad_ck_thermal(self, ISPACE, lp, lt, f_gas, taucont, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, **kw):
        self.calls.append(("cirsrad_ck_thermal", f_gas))
        return np.zeros((self.dims[0], np.shape(LAYINC)[1]))

    def cirsradg_ck_thermal(self, ISPACE, lp, lt, f_gas, taucont, dtaucon, NVMR, NPAR, igas_map, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, **kw):
        self.calls.append(("cirsradg_ck_thermal", igas_map))
        W, P = self.dims[0], np.shape(LAYINC)[1]
        return np.zeros((W, P)), np.zeros((W, NPAR, np.shape(LAYINC)[0], P)), np.zeros((W, P))

    def get_taugas(self, L, model=0):
        return np.zeros((self.dims[0], 1, L))

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture
def double(monkeypatch):
    e = RecordingEngine()
    monkeypatch.setattr(fm, "get_engine", lambda device=0: e)
    fm.reset_summary()
    yield e
    fm.reset_summary()


def test_line_source_from_line_data_applies_the_host_side_selections(golden):
    for name in oc.CASES:
        m, src = _model(golden, name)
        got, why = m._ansfm_line_source()
        assert why is None
        assert got.fingerprint() == src.fingerprint(), name                  # the far lines and bins were masked out again
    # include_pressure_shift = False zeroes the delta rows and nothing else
    m, src = _model(golden, "voigt_fm", include_pressure_shift=False)
    got = m._ansfm_line_source()[0]
    for a, b in zip(got.gases[0], src.gases[0]):
        assert not a.bparams[2::3].any() and np.array_equal(a.bparams[0::3], b.bparams[0::3]) and np.array_equal(a.bparams[1::3], b.bparams[1::3])
    assert got.fingerprint() != src.fingerprint()


@pytest.mark.parametrize("return_grad", [False, True])
def test_adapter_runs_ilbl_1_on_the_line_source(golden, double, return_grad):
    name = "voigt_fm"
    m, src = _model(golden, name)
    assert m._ansfm_supported(return_grad)
    out = m.CIRSrad(return_grad)
    assert double.names() == ["upload_line_source", "set_line_state", "cirsradg_ck_thermal" if return_grad else "cirsrad_ck_thermal"]
    st = double.calls[1][1]
    assert st.grad == return_grad and (st.n, st.L, st.S) == (1, m.LayerX.NLAY, src.S)
    assert np.array_equal(st.row_mix, np.repeat(_g(golden, name, "mix"), st.L, axis=0))          # amb_frac of :3822-3827
    assert np.array_equal(st.row_p_atm, np.tile(m.LayerX.PRESS / ATM, src.S))                    # PRESS / ATM_TO_PASCAL
    assert np.array_equal(st.row_q_lines[:4 * st.L].reshape(st.L, 4).T, _g(golden, name, "q_lines_g0"))
    if return_grad:
        assert np.array_equal(st.row_q_cont_dT[4 * st.L:], _g(golden, name, "q_cont_dT_g1")[0])
        assert len(out) == 3 and np.array_equal(double.calls[2][1], _g(golden, name, "igas"))
    else:
        assert np.array_equal(double.calls[2][1], np.ascontiguousarray(m.LayerX.AMOUNT[:, _g(golden, name, "igas")].T) * 1e-4)
    assert m.LayerX.TAUGAS.shape == (src.nw, 1, m.LayerX.NLAY)
    # the same line data again: the source stays in HBM, only the state is new
    m.CIRSrad(return_grad)
    assert double.names()[3:] == double.names()[1:3]
    s = fm.summary()
    assert s["delegated"] == {} and list(s["routes"].values()) == [2] and "ILBL = 1" in list(s["routes"])[0]
    # other line data: uploaded again
    m2, _ = _model(golden, "lorentz_fm")
    m2.CIRSrad(False)
    assert double.names()[5] == "upload_line_source"


def test_adapter_delegates_what_is_not_built(golden, double):
    ms = fm.IMOD_MULTIPLE_SCATTERING | 8192
    m, _ = _model(golden, "voigt_fm", imod=ms)
    assert m._ansfm_supported(False) and not m._ansfm_supported(True)         # the scattering branches have no gradients
    for change, reason in ((dict(lineshape=1), "line shape"), (dict(lineshape=6), "line shape")):
        m, _ = _model(golden, "voigt_fm", **change)
        assert not m._ansfm_supported(False) and reason in m._ansfm_line_source()[1]
    m, _ = _model(golden, "voigt_fm")
    m.SpectroscopyX.ISPACE = 1
    assert not m._ansfm_supported(False) and "wavelength" in m._ansfm_line_source()[1]
    m, _ = _model(golden, "voigt_fm")
    cd = m.SpectroscopyX.LINE_DATA[0].continuum_data[1]
    cd._data[1, 5] = -1.0                                                    # a bin width that is not positive
    assert not m._ansfm_supported(False) and "widths" in m._ansfm_line_source()[1]
    m, _ = _model(golden, "voigt_fm")
    del m.SpectroscopyX.LINE_DATA
    assert not m._ansfm_supported(False) and "LINE_DATA" in m._ansfm_line_source()[1]
    with pytest.warns(RuntimeWarning, match="runtime line-by-line"):
        with pytest.raises(NotImplementedError):                             # no reference class behind the mixin in this test
            m.CIRSrad(False)
    assert any("LINE_DATA" in k for k in fm.summary()["delegated"]) and double.calls == []
    fm.set_strict(True)
    try:
        with pytest.raises(NotImplementedError, match="strict"):
            m.CIRSrad(False)
    finally:
        fm.set_strict(False)
