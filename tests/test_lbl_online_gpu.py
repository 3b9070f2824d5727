"""CIRSrad on runtime line-by-line opacities (ILBL = 1) on the GPU: the line source resident in the context against the
reference's Spectroscopy_0.calc_klbl_online / calc_klblg_online and the ILBL = 1 branch of calculate_gaseous_line_opacity
(tests/golden/lbl_online.npz, tools/golden/gen_golden_lbl_online.py).

Tolerances.  k: rtol 1e-9, atol 1e-300, the project's tolerance for line and pseudo-continuum spectra (test_gpu_parity.py,
test_lbl_pc_gpu.py).  dkdT = (k(T + 5) - k(T)) / 5: within 1e-9 (2 |k| + 5 |dkdT|) / 5 -- two values each good to 1e-9 (k, and
k(T + 5) = k + 5 dkdT, at most |k| + 5 |dkdT|) allow their difference quotient that much.  TAUGAS / dTAUGAS: the same bounds
carried through the sum over the gases.  Radiances: the README's 1e-6 contract; gradients: 1e-4 of the column scale.
"""
import os

import numpy as np
import pytest

import lbl_online_cases as oc

pytestmark = pytest.mark.gpu
ATM = 101325.0
FM_CASES = [n for n, c in oc.CASES.items() if c["kind"] == "fm"]


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "lbl_online.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def sources(golden):
    return {name: oc.source_from_blob(golden, name + "__src_") for name in oc.CASES}


def _g(golden, name, key):
    return golden[f"{name}__{key}"]


def _rel(a, ref):
    m = ref != 0
    return float(np.max(np.abs(a[m] - ref[m]) / np.abs(ref[m])))


def _dk_bound(k, dkdT):
    return 1e-9 * (2 * np.abs(k) + 5 * np.abs(dkdT)) / 5


def _state(src, golden, name, grad):
    from archnemesis_dist_amd import line_source as ls
    return ls.pack_line_state(src, _g(golden, name, "PRESS") / ATM, _g(golden, name, "TEMP"), _g(golden, name, "mix"), grad=grad)


def _amount(golden, name):
    """(S, L) columns in m-2 as the engine takes them (:3838)"""
    return np.ascontiguousarray(_g(golden, name, "AMOUNT")[:, _g(golden, name, "igas")].T) * 1.0e-4


# ---- a: the seams ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.CASES))
def test_seams_against_the_reference(eng, golden, sources, name):
    src = sources[name]
    eng.upload_line_source(src)
    assert eng.ktable_info()[0] == (src.nw, 1, 2, 2, src.S)                 # answers like an LBL table with G = 1, W = nw
    p, t, amb = _g(golden, name, "PRESS") / ATM, _g(golden, name, "TEMP"), _g(golden, name, "amb_frac")
    k = eng.calc_klbl_online(p, t, amb)
    kg, dk = eng.calc_klbl_online(p, t, amb, grad=True)
    ref_k, ref_dk = _g(golden, name, "k"), _g(golden, name, "dkdT")
    assert np.array_equal(k, kg)                                            # one sum order for both seams
    nz = ref_k != 0
    print(f"{name}: k max rel err {_rel(kg, ref_k):.3e}; dkdT max err / bound "
          f"{np.max(np.abs(dk - ref_dk)[nz] / _dk_bound(ref_k, ref_dk)[nz]):.3e}")
    np.testing.assert_allclose(kg, ref_k, rtol=1e-9, atol=1e-300)
    assert np.all(np.abs(dk - ref_dk) <= _dk_bound(ref_k, ref_dk))
    if f"{name}__k_fwd" in golden:                                          # calc_klbl_online's own order: to rounding only
        np.testing.assert_allclose(k, _g(golden, name, "k_fwd"), rtol=1e-9, atol=1e-300)


# ---- b: TAUGAS / dTAUGAS of a CIRSrad call -------------------------------------------------------------------------------
def _nadir(L, W):
    from archnemesis_dist_amd import synthetic as syn
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, 20.0)
    return NLAYIN, LAYINC, SCALE, syn.synth_continuum(W, L)[0]


@pytest.mark.parametrize("name", FM_CASES)
def test_taugas_side_products_against_the_reference(eng, golden, sources, name):
    src = sources[name]
    eng.upload_line_source(src)
    lp, lt, am = _g(golden, name, "PRESS"), _g(golden, name, "TEMP"), _amount(golden, name)
    L, W, S = lp.size, src.nw, src.S
    NLAYIN, LAYINC, SCALE, cont = _nadir(L, W)
    EMTEMP = lt[LAYINC[:, 0]][:, None]
    ref_tau, ref_d, igas = _g(golden, name, "TAUGAS"), _g(golden, name, "dTAUGAS"), _g(golden, name, "igas")
    NVMR = ref_d.shape[2] - 2
    eng.set_line_state(_state(src, golden, name, grad=False))
    eng.cirsrad_ck_thermal(0, lp, lt, am, cont, NLAYIN, LAYINC, SCALE, EMTEMP, -1.0)
    tau_f = eng.get_taugas(L, 0)
    eng.set_line_state(_state(src, golden, name, grad=True))
    eng.cirsradg_ck_thermal(0, lp, lt, am, cont, None, NVMR, NVMR + 2, igas.astype(np.int32), NLAYIN, LAYINC, SCALE, EMTEMP, -1.0)
    tau_g, d = eng.get_taugas(L, 0), eng.get_dtaugas(L, 0)
    assert np.array_equal(tau_f, tau_g)
    print(f"{name}: TAUGAS max rel err {_rel(tau_g, ref_tau):.3e}")
    np.testing.assert_allclose(tau_g, ref_tau, rtol=1e-9, atol=1e-300)
    ref_k, ref_dk = _g(golden, name, "k"), _g(golden, name, "dkdT")
    for s in range(S):                                                      # :3844
        np.testing.assert_allclose(d[:, 0, s, :] * 1.0e-4, ref_d[:, 0, igas[s], :], rtol=1e-9, atol=1e-300)
    bound = sum(_dk_bound(ref_k[:, :, s], ref_dk[:, :, s]) * am[s][None, :] for s in range(S))
    err = np.abs(d[:, 0, S, :] - ref_d[:, 0, NVMR, :])                      # :3845
    print(f"{name}: dTAUGAS/dT max err / bound {np.max(err[bound > 0] / bound[bound > 0]):.3e}")
    assert np.all(err <= bound)
    assert not ref_d[:, 0, [i for i in range(NVMR + 2) if i not in list(igas) + [NVMR]], :].any()


@pytest.mark.parametrize("name", FM_CASES)
def test_cirsrad_mixin_runs_ilbl_1_on_the_gpu(golden, name):
    """CIRSradGPU.CIRSrad on a model whose SpectroscopyX carries LINE_DATA (stand-ins read like LineData_0): the TAUGAS side
    product against the reference's, the radiance with and without gradients, nothing delegated."""
    from archnemesis_dist_amd import forward_model as fm
    from test_lbl_online_host import _model
    fm.reset_summary()
    m, src = _model(golden, name)
    out = m.CIRSrad(False)
    np.testing.assert_allclose(m.LayerX.TAUGAS, _g(golden, name, "TAUGAS"), rtol=1e-9, atol=1e-300)
    spec, dspec, dts = m.CIRSrad(True)
    np.testing.assert_allclose(m.LayerX.TAUGAS, _g(golden, name, "TAUGAS"), rtol=1e-9, atol=1e-300)
    np.testing.assert_allclose(spec, out, rtol=1e-12)
    assert out.shape == (src.nw, 1) and np.all(out > 0) and dspec.shape == (src.nw, 5, m.LayerX.NLAY, 1) and dspec[:, :2].any()
    s = fm.summary()
    assert s["delegated"] == {} and list(s["routes"].values()) == [2]
    fm.reset_summary()


# ---- c: radiative transfer on the line source against the oracle's RT fed the reference's TAUGAS -------------------------------
def _paths(L):
    """a nadir path and a limb-like one: fewer layers, each crossed twice as long"""
    P = 2
    LAYINC = np.zeros((L, P), dtype=np.int32)
    LAYINC[:, 0] = np.arange(L - 1, -1, -1); LAYINC[:L - 1, 1] = np.arange(L - 1, 0, -1)
    NLAYIN = np.array([L, L - 1], dtype=np.int32)
    SCALE = np.where(np.arange(L)[:, None] < NLAYIN[None, :], np.array([1.0 / np.cos(np.deg2rad(25.0)), 7.5])[None, :], 0.0)
    return NLAYIN, LAYINC, SCALE


def test_thermal_and_transmission_against_the_oracle(eng, oracle, golden, sources):
    name = "voigt_fm"
    src = sources[name]
    eng.upload_line_source(src)
    lp, lt, am = _g(golden, name, "PRESS"), _g(golden, name, "TEMP"), _amount(golden, name)
    L, W, S = lp.size, src.nw, src.S
    WAVE = src.wn_grid
    from archnemesis_dist_amd import synthetic as syn
    cont = syn.synth_continuum(W, L)[0]
    NLAYIN, LAYINC, SCALE = _paths(L)
    EMTEMP = np.where(np.arange(L)[:, None] < NLAYIN[None, :], lt[LAYINC], 0.0)
    ref_tau, ref_d, igas = _g(golden, name, "TAUGAS"), _g(golden, name, "dTAUGAS"), _g(golden, name, "igas").astype(np.int32)
    NVMR = ref_d.shape[2] - 2
    NPAR = NVMR + 2
    tautot = ref_tau[:, 0, :] + cont
    z, one = np.zeros(W), np.ones(W)
    eng.set_line_state(_state(src, golden, name, grad=True))
    out = eng.cirsrad_ck_thermal(0, lp, lt, am, cont, NLAYIN, LAYINC, SCALE, EMTEMP, 250.0, EMISSIVITY=one)
    spec, dspec, dts = eng.cirsradg_ck_thermal(0, lp, lt, am, cont, None, NVMR, NPAR, igas, NLAYIN, LAYINC, SCALE, EMTEMP, 250.0,
                                               EMISSIVITY=one)
    tr = eng.cirsrad_ck_transmission(lp, lt, am, cont, NLAYIN, LAYINC, SCALE)
    trg, dtr = eng.cirsradg_ck_transmission(lp, lt, am, cont, None, NVMR, NPAR, igas, NLAYIN, LAYINC, SCALE)
    worst = {}
    for ip in range(2):
        n = int(NLAYIN[ip]); li = LAYINC[:n, ip]
        path = (tautot[:, li] * SCALE[:n, ip])[:, None, :]
        dpath = ref_d[:, :, :, li] * SCALE[:n, ip]
        rs, rd, rt = oracle.calc_thermal_emission_spectrumg(0, WAVE, path, dpath, NVMR, EMTEMP[:n, ip], lp[li], 250.0, one)
        ref = oracle.calc_thermal_emission_spectrum(0, WAVE, path, None, EMTEMP[:n, ip], lp[li], 250.0, one, z, z, 180.0, 180.0)
        worst[f"thermal p{ip}"] = np.max(np.abs(out[:, ip] - ref[:, 0]) / np.abs(ref[:, 0]))
        worst[f"thermal (gradient call) p{ip}"] = np.max(np.abs(spec[:, ip] - rs[:, 0]) / np.abs(rs[:, 0]))
        scale = np.abs(rd[:, 0]).max(axis=(0, 2), keepdims=True) + 1e-300
        worst[f"d thermal p{ip}"] = np.max(np.abs(dspec[:, :, :n, ip] - rd[:, 0]) / scale)
        worst[f"dTSURF p{ip}"] = np.max(np.abs(dts[:, ip] - rt[:, 0])) / np.abs(rt).max()
        t_ref = np.exp(-path[:, 0, :].sum(axis=1))
        worst[f"transmission p{ip}"] = np.max(np.abs(tr[:, ip] - t_ref) / t_ref)
        d_ref = -t_ref[:, None, None] * dpath[:, 0]                          # (W, NPAR, n)
        scale = np.abs(d_ref).max(axis=(0, 2), keepdims=True) + 1e-300
        worst[f"d transmission p{ip}"] = np.max(np.abs(dtr[:, :, :n, ip] - d_ref) / scale)
    print({k: f"{v:.2e}" for k, v in worst.items()})
    np.testing.assert_allclose(trg, tr, rtol=1e-12)
    for k, v in worst.items():
        assert v < (1e-4 if k.startswith("d") else 1e-6), (k, v)
    assert np.ptp(ref_tau[:, 0, :].sum(axis=1)) > 1.0                       # the lines shape the spectrum


def test_single_scattering_against_the_oracle(eng, oracle, golden, sources):
    import singlescatt_cases as sc
    name = "voigt_fm"
    src = sources[name]
    eng.upload_line_source(src)
    lp, lt, am = _g(golden, name, "PRESS"), _g(golden, name, "TEMP"), _amount(golden, name)
    L, W = lp.size, src.nw
    rng = np.random.default_rng(5)
    cont = 10.0 ** rng.uniform(-3, -1.5, (W, L)); sca = cont * rng.uniform(0.3, 0.9, (W, L))
    NLAYIN, LAYINC, SCALE = _paths(L)
    EMTEMP = np.where(np.arange(L)[:, None] < NLAYIN[None, :], lt[LAYINC], 0.0)
    phase = 10.0 ** rng.uniform(-1.5, 0.3, (2, W, L))
    sol, emi = np.array([30.0, 55.0]), np.array([25.0, 40.0])
    EMIS, BRDF, SOLF = rng.uniform(0.7, 1.0, W), rng.uniform(0.02, 0.15, (W, 2)), 10.0 ** rng.uniform(-8, -7, W)
    eng.set_line_state(_state(src, golden, name, grad=False))
    out = eng.cirsrad_ck_singlescatt(0, lp, lt, am, cont, sca, phase, NLAYIN, LAYINC, SCALE, EMTEMP, 240.0, EMIS, BRDF, SOLF, sol, emi)
    tautot = _g(golden, name, "TAUGAS") + cont[:, None, :]
    omega = sca[:, None, :] / tautot
    ref = np.zeros((W, 2))
    for ip in range(2):
        n = int(NLAYIN[ip]); li = LAYINC[:n, ip]
        ref[:, ip] = oracle.calc_singlescatt_plane_spectrum(0, src.wn_grid, tautot[:, :, li] * SCALE[:n, ip], EMTEMP[:n, ip], omega[:, :, li],
                                                            phase[ip][:, li], 240.0, EMIS, BRDF[:, ip], SOLF, sol[ip], emi[ip])[:, 0]
    err = np.max(np.abs(out - ref) / np.abs(ref))
    print(f"single scattering max rel err {err:.2e}")
    assert err < 1e-6


@pytest.mark.parametrize("NMU,NF,up", [(5, 2, False), (16, 3, True)])
def test_multiple_scattering_against_the_oracle(eng, oracle, golden, sources, monkeypatch, NMU, NF, up):
    from test_lbl_scatter import _geometry, _lbl_inputs, _scatter
    name = "voigt_fm"
    src = sources[name]
    eng.upload_line_source(src)
    lp, lt, am = _g(golden, name, "PRESS"), _g(golden, name, "TEMP"), _amount(golden, name)
    L, W, S = lp.size, src.nw, src.S
    z = _lbl_inputs(np.random.default_rng(4100 + NMU), W, L, S, NMU, NF, 1, 1, 1, 1)
    wave = src.wn_grid
    c1, c2 = 1.1911e-12, 1.439
    z.update(WAVE=wave, lay_p=lp, lay_t=lt, amount=am,
             radg=np.repeat((c1 * wave ** 3 / (np.exp(c2 * wave / lt[0]) - 1.0))[:, None], NMU, 1))
    eng.set_line_state(_state(src, golden, name, grad=False))
    out, spec_g = _scatter(eng, z, up, spec_g=True)
    assert eng.last_scatter_windows() == (1, W)
    monkeypatch.setenv("ANSFM_MS_WINDOW", "192")                            # a G = 1 window smaller than nw changes no bit
    out_w, spec_w = _scatter(eng, z, up, spec_g=True)
    assert eng.last_scatter_windows() == (-(-W // 192), 192)
    assert np.array_equal(out, out_w) and np.array_equal(spec_g, spec_w)
    sol, emi, azi = _geometry(up)
    taugas = _g(golden, name, "TAUGAS")
    tautot = taugas + (z["TAUCIA"] + z["TAUDUST"] + z["TAURAY"])[:, None, :]
    omega = (z["TAURAY"] + z["TAUSCAT"])[:, None, :] / tautot
    bnu = c1 * wave[:, None] ** 3 / (np.exp(c2 * wave[:, None] / lt[None, :]) - 1.0)
    rad = oracle.scloud11wave_core(z["phasarr"], z["radg"], sol, emi, z["solar"], azi, z["lowbc"], z["brdf"], z["MU"], z["WT"], NF, wave,
                                   bnu, tautot, z["TAURAY"], omega, 101, 1, 1, z["lfrac"])
    ref = np.transpose(rad, (2, 1, 0))[:, 0, :]
    err = np.max(np.abs(out - ref) / np.abs(ref))
    print(f"multiple scattering, {NMU} streams: max rel err {err:.2e}")
    np.testing.assert_allclose(eng.get_taugas(L, 0), taugas, rtol=1e-9, atol=1e-300)
    assert err < 1e-6


# ---- d: a batch by distinct rows ------------------------------------------------------------------------------------------------
def _four_states(golden, name):
    """state 0; one temperature level perturbed; gas 0 scaled, so that its amb_frac changes; a copy of state 0"""
    from archnemesis_dist_amd import line_source as ls
    lp, lt = np.repeat(_g(golden, name, "PRESS")[None], 4, 0), np.repeat(_g(golden, name, "TEMP")[None], 4, 0)
    am = np.repeat(_amount(golden, name)[None], 4, 0)
    PP = np.repeat(_g(golden, name, "PP")[None], 4, 0)
    lt[1, 2] += 1.5
    am[2, 0] *= 1.1; PP[2, :, 0] *= 1.1
    spec_ids = [g[0] for g in oc.GASES]
    mix = np.stack([ls.mix_fractions(ls.ambient_fractions(PP[m], lp[m], _g(golden, name, "ATM_ID"), spec_ids)) for m in range(4)])
    return lp, lt, am, mix


@pytest.mark.parametrize("grad", [False, True])
def test_batch_of_four_states_equals_single_calls(eng, golden, sources, grad):
    from archnemesis_dist_amd import line_source as ls
    name = "voigt_fm"
    src = sources[name]
    eng.upload_line_source(src)
    lp, lt, am, mix = _four_states(golden, name)
    n, L = lp.shape
    W, S = src.nw, src.S
    NLAYIN, LAYINC, SCALE, cont = _nadir(L, W)
    EMTEMP = np.stack([lt[m][LAYINC[:, 0]][:, None] for m in range(n)])
    SC = np.repeat(SCALE[None], n, 0)
    conts = np.repeat(cont[None], n, 0)
    TS = np.full(n, 250.0)
    igas = np.arange(S, dtype=np.int32)

    def call(sel):
        if grad:
            return eng.cirsradg_ck_thermal(0, lp[sel], lt[sel], am[sel], conts[sel], None, S, S + 2, igas, NLAYIN, LAYINC, SC[sel],
                                           EMTEMP[sel], TS[sel] if lp[sel].ndim == 2 else 250.0, EMISSIVITY=np.ones(W))
        return (eng.cirsrad_ck_thermal(0, lp[sel], lt[sel], am[sel], conts[sel], NLAYIN, LAYINC, SC[sel], EMTEMP[sel],
                                       TS[sel] if lp[sel].ndim == 2 else 250.0, EMISSIVITY=np.ones(W)),)

    st = ls.pack_line_state(src, lp / ATM, lt, mix, grad=grad)
    # the packer's count: gas 0 changes in every layer of state 2, both gases in the perturbed layer of state 1
    assert st.R == S * L + S * 1 + L and np.array_equal(st.krow[3], st.krow[0])
    eng.set_line_state(st)
    batch = call(slice(None))
    assert eng.last_line_rows()[:2] == (st.R, st.R * (2 if grad else 1))
    taus = [eng.get_taugas(L, m) for m in range(n)]
    eng.set_line_scratch_bytes(64 * 1024)                                    # a few rows per chunk
    eng.set_line_state(st)
    chunked = call(slice(None))
    assert eng.last_line_rows()[2] > S
    eng.set_line_scratch_bytes(256 << 20)
    for a, b in zip(batch, chunked):
        assert np.array_equal(a, b)
    for m in range(n):
        eng.set_line_state(ls.pack_line_state(src, lp[m] / ATM, lt[m], mix[m], grad=grad))
        single = call(m)
        for a, b in zip(batch, single):
            assert np.array_equal(a[m], b), m
        assert np.array_equal(eng.get_taugas(L, 0), taus[m])
    assert np.array_equal(batch[0][3], batch[0][0]) and not np.array_equal(batch[0][1], batch[0][0]) \
        and not np.array_equal(batch[0][2], batch[0][0])


def test_scatter_batch_on_the_line_source_equals_single_calls(eng, golden, sources):
    """ansfm_cirsrad_ck_scatter_batch in runtime mode: no layer cache (its comparison does not see the mix fractions), the
    models one by one, each reading its own rows of the state"""
    from archnemesis_dist_amd import line_source as ls
    from test_lbl_scatter import _geometry, _lbl_inputs
    name = "voigt_fm"
    src = sources[name]
    eng.upload_line_source(src)
    lp, lt, am, mix = (a[:3] for a in _four_states(golden, name))
    n, L = lp.shape
    W, S, NMU, NF = src.nw, src.S, 5, 2
    z = _lbl_inputs(np.random.default_rng(4300), W, L, S, NMU, NF, 1, 1, 1, 1)
    rep = lambda a: np.repeat(np.asarray(a)[None], n, 0).copy()
    cia, dust, ray, sca, lf, rg = (rep(z[k]) for k in ("TAUCIA", "TAUDUST", "TAURAY", "TAUSCAT", "lfrac", "radg"))
    sol, emi, azi = _geometry(False)
    tail = (sol, emi, azi, z["solar"], 1, z["brdf"], z["MU"], z["WT"], NF, 101, 1, 1)
    eng.set_line_state(ls.pack_line_state(src, lp / ATM, lt, mix))
    got = eng.cirsrad_ck_scatter_batch(0, lp, lt, am, cia, dust, ray, sca, z["phasarr"], lf, rg, *tail)
    assert eng.last_scatter_cache()[0] == 0
    for m in range(n):
        eng.set_line_state(ls.pack_line_state(src, lp[m] / ATM, lt[m], mix[m]))
        one = eng.cirsrad_ck_scatter(0, lp[m], lt[m], am[m], cia[m], dust[m], ray[m], sca[m], z["phasarr"], lf[m], rg[m], *tail)
        assert np.array_equal(got[m], one), m
    assert not np.array_equal(got[1], got[0]) and not np.array_equal(got[2], got[0])


# ---- e: the line source against the accumulator ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.CASES))
def test_rows_equal_the_accumulator_bit_for_bit(eng, golden, sources, name):
    from archnemesis_dist_amd import line_source as ls
    src = sources[name]
    p, t, mix = _g(golden, name, "PRESS") / ATM, _g(golden, name, "TEMP"), _g(golden, name, "mix")
    L = p.size
    eng.upload_line_source(src)
    k = eng.calc_klbl_online(p, t, _g(golden, name, "amb_frac"))
    for s, isos in enumerate(src.gases):
        ql, qc = ls.q_ratios(src, np.full(L, s), t)
        ql, qc = ql.reshape(L, -1), qc.reshape(L, -1)
        acc = eng.lbl_accumulator(src.wn_grid, t, p)
        for i, iso in enumerate(isos):
            if iso.include_lines and iso.N:
                acc.add_lines(iso.lineshape_id, iso.t_ref, iso.p_ref, ql[:, i], iso.abundance, iso.mass, mix[s], iso.bparams, iso.nu, iso.sw,
                              iso.e_lower, iso.stim_ref, s_floor=iso.s_floor, wn_calc_window=iso.wn_calc_window,
                              wn_approx_window=iso.wn_approx_window)
            if iso.include_continuum and iso.Nb:
                acc.add_pseudo_continuum(iso.lineshape_id, iso.t_cont, iso.p_cont, qc[:, i], iso.abundance, iso.mass, mix[s],
                                         iso.pc_bparams, iso.centers, iso.widths, iso.sw_sum, iso.pc_e_lower,
                                         n_neighbour_bins=iso.n_neighbour_bins)
        assert np.array_equal(acc.numpy().T, k[:, :, s]), (name, s)


# ---- the mode and its errors on the device --------------------------------------------------------------------------------------
def test_mode_changes_and_error_codes(eng, golden, sources):
    from archnemesis_dist_amd import line_source as ls
    name = "lorentz_fm"
    src = sources[name]
    lp, lt, am = _g(golden, name, "PRESS"), _g(golden, name, "TEMP"), _amount(golden, name)
    L, W = lp.size, src.nw
    NLAYIN, LAYINC, SCALE, cont = _nadir(L, W)
    EMTEMP = lt[LAYINC[:, 0]][:, None]
    thermal = lambda: eng.cirsrad_ck_thermal(0, lp, lt, am, cont, NLAYIN, LAYINC, SCALE, EMTEMP, -1.0)
    eng.upload_line_source(src)
    with pytest.raises(ValueError, match="set_state"):                       # a call before any state
        thermal()
    st = _state(src, golden, name, grad=False)
    eng.set_line_state(st)
    a = thermal()
    with pytest.raises(ValueError, match="does not match"):                  # (n, L) of the call differs from the state's
        eng.cirsrad_ck_thermal(0, lp[:-1], lt[:-1], am[:, :-1], cont[:, :-1], *_nadir(L - 1, W)[:3], EMTEMP[:-1], -1.0)
    with pytest.raises(ValueError, match="T \\+ 5 K"):                       # a gradient call on a state without the _dT ratios
        eng.cirsradg_ck_thermal(0, lp, lt, am, cont, None, 2, 4, np.arange(2, dtype=np.int32), NLAYIN, LAYINC, SCALE, EMTEMP, -1.0)
    bad = _state(src, golden, name, grad=False)
    bad.krow[0, 1, 0] = bad.krow[0, 0, 0]                                    # a row of another gas
    with pytest.raises(ValueError, match="krow\\[0\\]\\[1\\]\\[0\\]"):
        eng.set_line_state(bad)
    bad.krow[0, 1, 0] = st.R
    with pytest.raises(ValueError, match="outside"):
        eng.set_line_state(bad)
    with pytest.raises(_lib_error()):                                        # the table seams do not answer in this mode
        eng.calc_klbl(lp / ATM, lt)
    # a table leaves the mode, a new commit comes back to it
    from archnemesis_dist_amd import synthetic as syn
    PRESS, TEMP, K = syn.synth_ktable(W, 4, 6, 4, src.S, seed=5)
    eng.upload_ktable(K, PRESS, TEMP, src.wn_grid, syn.gauss_legendre_01(4)[1])
    thermal()                                                                # no state needed: the table answers
    with pytest.raises(ValueError, match="commit a line source"):
        eng.set_line_state(st)
    eng.upload_line_source(src)
    eng.set_line_state(st)
    assert np.array_equal(thermal(), a)
    # argument checks of the isotopologue entry: the line and pseudo-continuum entries' codes
    iso = src.gases[0][0]
    import copy
    for change, exc in ((dict(lineshape_id=3), NotImplementedError), (dict(n_neighbour_bins=9), NotImplementedError),
                        (dict(centers=iso.centers[::-1].copy()), ValueError)):
        b = copy.copy(iso)
        b.__dict__.update(change)
        with pytest.raises(exc):
            eng.upload_line_source(ls.LineSource(src.wn_grid, [[b]] + src.gases[1:], src.M))
    with pytest.raises(ValueError):                                          # a descending grid
        eng.upload_line_source(ls.LineSource(src.wn_grid[::-1].copy(), src.gases, src.M))


def _lib_error():
    from archnemesis_dist_amd import _lib
    return _lib.AnsfmError
