"""CIA and aerosol continuum of a Jacobian batch formed inside the batched thermal call, per distinct layer, from sources
resident in the context (ansfm_upload_cia / ansfm_upload_dust / ansfm_cirsrad_ck_thermal_cont_dev): bit identity with the
route through calc_tau_cia / calc_tau_dust / calc_tau_rayleigh_batch_dev and a dense taucont, the oracle, the model level
(profile_state.BatchedCKThermalModel) and the refusals."""
import os

import numpy as np
import pytest

from test_cia_oracle import cia_args

pytestmark = pytest.mark.gpu

W, G, S, L, NVMR, N = 150, 10, 4, 9, 6, 6          # W = 150 is no multiple of the wavenumber tile: W != Wpad
NP_T, NT_T = 6, 5


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "tau_cia.npz"))


def cia_tables(z, tag):
    """the layer-independent arguments of calc_tau_cia from the golden file: CIA_WAVEN .. INORMALD"""
    a, _ = cia_args(z, tag, 0)
    return a[2:12]


def grid(ISPACE):
    # inside the CIA table's wavenumbers (0 .. 6000 cm-1) in either space
    return 100.0 + 20.0 * np.arange(W) if ISPACE == 0 else np.linspace(1.8, 60.0, W)


def batch(z, NDUST, seed=3):
    """N states of L layers: state 0 from the golden file's layers, every other state differs from it in exactly one layer
    -- in temperature, only in He's mixing ratio, only in DELH, only in FRAC, only in CONT."""
    from archnemesis_dist_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    ID, ISO = syn.PROFILE_GAS_ID[:NVMR].copy(), np.zeros(NVMR, dtype=np.int32)       # 39, 40, 6, 11, 26, 27
    rep = lambda a: np.repeat(np.asarray(a, float)[None], N, 0)
    PRESS, TEMP, FRAC, TOTAM, DELH = (rep(z[k]) for k in ("PRESS", "TEMP", "FRAC", "TOTAM", "DELH"))
    q0 = np.empty((L, NVMR))
    q0[:, 2:] = 10.0 ** rng.uniform(-6, -3, (L, NVMR - 2))
    rest = 1.0 - q0[:, 2:].sum(1)
    q0[:, 0], q0[:, 1] = 0.864 * rest, 0.136 * rest
    PP = rep(q0 * PRESS[0][:, None])
    CONT = rep(10.0 ** rng.uniform(8, 10, (L, max(NDUST, 1))))[:, :, :NDUST]
    if NDUST:
        CONT[:, 1, NDUST - 1] = -3.0e9                # clipped to zero (:3966)
    TEMP[1, 3] *= 1.05
    PP[2, 4, 1] *= 1.05                               # He: no spectroscopic amount changes, CIA does
    DELH[3, 2] *= 1.05
    FRAC[4, 5] += 0.03
    if NDUST:
        CONT[5, 6, 0] *= 1.05
    q = PP / PRESS[:, :, None]                        # Layer_0: what calc_tau_cia forms from PP and PRESS
    amount = np.ascontiguousarray(np.transpose(q[:, :, 2:2 + S] * TOTAM[:, :, None], (0, 2, 1))) * 1.0e-4
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, 20.0)
    return dict(ID=ID, ISO=ISO, PRESS=PRESS, TEMP=TEMP, FRAC=FRAC, TOTAM=TOTAM, DELH=DELH, PP=PP, q=q, CONT=CONT, amount=amount,
                NLAYIN=NLAYIN, LAYINC=LAYINC, SCALE=SCALE, EMTEMP=np.ascontiguousarray(TEMP[:, LAYINC[:, 0]][:, :, None]))


def dust_table(WAVE, NDUST):
    """KEXT / KSCA (NWS, NDUST) on a grid of 12 points around WAVE"""
    SWAVE = np.linspace(WAVE.min() * 0.9, WAVE.max() * 1.1, 12)
    x = np.linspace(0.0, 1.0, 12)[:, None]
    KEXT = 1.0e-9 * (1.0 + 0.6 * np.sin(5.0 * x + np.arange(NDUST)[None])) * (1.0 + np.arange(NDUST)[None])
    return SWAVE, KEXT, 0.7 * KEXT * (1.0 - 0.5 * x)


def ktable(WAVE):
    from archnemesis_dist_amd import synthetic as syn
    TPRESS, TTEMP, K = syn.synth_ktable(W, G, NP_T, NT_T, S, seed=41)
    _, delg = syn.gauss_legendre_01(G)
    return K, TPRESS, TTEMP, WAVE, delg


def distinct_rows(b, cols):
    """rows the de-duplication computes: state 0's L and every layer of another state that differs from state 0's in a byte"""
    ident = np.concatenate([np.ascontiguousarray(c, dtype=np.float64).reshape(N, L, -1) for c in cols], axis=2)
    by = np.ascontiguousarray(ident).view(np.uint8).reshape(N, L, -1)
    return L + int(np.sum(np.any(by[1:] != by[:1], axis=2)))


def fused(eng, b, ISPACE, IRAY, NDUST, sel=slice(None)):
    import torch
    dev = torch.device("cuda", eng.device)
    td = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    n = b["PRESS"][sel].shape[0]
    out = torch.empty((n, W, 1), dtype=torch.float64, device=dev)
    f4 = td(eng.rayleigh_f4(b["ID"], b["ISO"], b["q"][sel])) if IRAY == 4 else None
    torch.cuda.current_stream(dev).synchronize()
    eng.cirsrad_ck_thermal_cont_dev(ISPACE, n, L, td(b["PRESS"][sel]), td(b["TEMP"][sel]), td(b["amount"][sel]), td(b["q"][sel]),
                                    td(b["FRAC"][sel]), td(b["TOTAM"][sel]), td(b["DELH"][sel]),
                                    td(b["CONT"][sel]) if NDUST else None, IRAY, f4, 1, L, td(b["NLAYIN"], torch.int32),
                                    td(b["LAYINC"], torch.int32), td(np.repeat(b["SCALE"][None], n, 0)), td(b["EMTEMP"][sel]),
                                    td(np.full(n, -1.0)), None, None, None, None, None, None, out)
    eng.synchronize()
    return out.cpu().numpy()


def dense(eng, b, tabs, dust, ISPACE, WAVE, IRAY, NDUST):
    """the two-call route: the continuum of all N * L layers from the array-level entries, summed as (cia + dust) + ray"""
    import torch
    dev = torch.device("cuda", eng.device)
    td = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    flat = lambda a: np.ascontiguousarray(a).reshape((N * L,) + a.shape[2:])
    host = eng.calc_tau_cia(ISPACE, WAVE, *tabs, b["ID"], b["ISO"], flat(b["PP"]), flat(b["PRESS"]), flat(b["TEMP"]), flat(b["FRAC"]),
                            flat(b["TOTAM"]), flat(b["DELH"]), with_grad=False)
    if NDUST:
        t = eng.calc_tau_dust(WAVE, *dust, flat(b["CONT"]))[0]
        host = host + np.sum(np.clip(np.nan_to_num(t), 0, 1e20), 2)
    cont = td(np.transpose(host.reshape(W, N, L), (1, 0, 2)))
    if IRAY:
        ray = torch.empty((N, W, L), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        eng.calc_tau_rayleigh_batch_dev(IRAY, ISPACE, b["TOTAM"], ray, ID=b["ID"], ISO=b["ISO"], VMR=b["q"])
        eng.synchronize()
        cont = cont + ray
    out = torch.empty((N, W, 1), dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    eng.cirsrad_ck_thermal_dev(ISPACE, N, L, td(b["PRESS"]), td(b["TEMP"]), td(b["amount"]), cont, 1, L, td(b["NLAYIN"], torch.int32),
                               td(b["LAYINC"], torch.int32), td(np.repeat(b["SCALE"][None], N, 0)), td(b["EMTEMP"]),
                               td(np.full(N, -1.0)), None, None, None, None, None, None, out)
    eng.synchronize()
    return out.cpu().numpy()


def sources(eng, tabs, b, ISPACE, WAVE, NDUST):
    eng.upload_ktable(*ktable(WAVE))
    eng.upload_cia(ISPACE, WAVE, *tabs, b["ID"], b["ISO"])
    dust = dust_table(WAVE, NDUST) if NDUST else None
    if NDUST:
        eng.upload_dust(*dust)
    return dust


@pytest.mark.parametrize("NDUST", [0, 2])
@pytest.mark.parametrize("IRAY", [0, 4, 1])             # IRAY 4's opacity is below an ulp of TAUCIA here; IRAY 1's is not
@pytest.mark.parametrize("ISPACE", [0, 1])
@pytest.mark.parametrize("tag", ["normal", "para"])
def test_fused_continuum_is_bit_identical_with_the_two_call_route(eng, golden, tag, ISPACE, IRAY, NDUST):
    tabs, WAVE, b = cia_tables(golden, tag), grid(ISPACE), batch(golden, NDUST)
    dust = sources(eng, tabs, b, ISPACE, WAVE, NDUST)
    eng.set_layer_dedup(True)
    ref = dense(eng, b, tabs, dust, ISPACE, WAVE, IRAY, NDUST)
    assert np.all(np.isfinite(ref)) and ref.min() > 0.0
    # every state's spectrum differs from state 0's (the He-only one through CIA alone when there is no Rayleigh term), except
    # where its layer differs in what the case does not use: FRAC without a para-H2 axis, CONT without aerosols
    for i in range(1, N):
        unused = (i == 4 and tag == "normal") or (i == 5 and not NDUST)
        assert np.array_equal(ref[i], ref[0]) == unused, i
    got = fused(eng, b, ISPACE, IRAY, NDUST)
    assert np.array_equal(got, ref)
    cols = [b["PRESS"], b["TEMP"], np.transpose(b["amount"], (0, 2, 1)), b["q"], b["FRAC"], b["TOTAM"], b["DELH"]]
    cols += [b["CONT"]] if NDUST else []
    cols += [eng.rayleigh_f4(b["ID"], b["ISO"], b["q"])] if IRAY == 4 else []
    want = distinct_rows(b, cols)
    assert want == L + (5 if NDUST else 4)
    assert eng.last_layer_rows() == (want, N * L)
    try:
        eng.set_layer_dedup(False)
        assert np.array_equal(fused(eng, b, ISPACE, IRAY, NDUST), ref)
        assert eng.last_layer_rows() == (N * L, N * L)
    finally:
        eng.set_layer_dedup(True)
    for i in (0, 2):                                   # one state per call: no de-duplication, no row list
        assert np.array_equal(fused(eng, b, ISPACE, IRAY, NDUST, sel=slice(i, i + 1))[0], ref[i])


@pytest.mark.parametrize("IRAY", [4, 1])
@pytest.mark.parametrize("ISPACE", [0, 1])
@pytest.mark.parametrize("tag", ["normal", "para"])
def test_fused_continuum_against_the_oracle(eng, oracle, golden, tag, ISPACE, IRAY):
    """per state: oracle.calc_tau_cia + calc_tau_dust + calc_tau_rayleigh, then oracle.cirsrad_ck_thermal; rtol 1e-10, the
    bound of the thermal spectra against the oracle in test_gpu_parity.py"""
    NDUST = 2
    tabs, WAVE, b = cia_tables(golden, tag), grid(ISPACE), batch(golden, NDUST)
    dust = sources(eng, tabs, b, ISPACE, WAVE, NDUST)
    got = fused(eng, b, ISPACE, IRAY, NDUST)
    K, TPRESS, TTEMP, _, delg = ktable(WAVE)
    for i in range(N):
        cia = oracle.calc_tau_cia(ISPACE, WAVE, *tabs, b["ID"], b["ISO"], b["PP"][i], b["PRESS"][i], b["TEMP"][i], b["FRAC"][i],
                                  b["TOTAM"][i], b["DELH"][i])[0]
        td1 = oracle.calc_tau_dust(WAVE, *dust, b["CONT"][i])[0]
        ray = oracle.calc_tau_rayleigh(IRAY, ISPACE, WAVE, b["TOTAM"][i], ID=b["ID"], ISO=b["ISO"], VMR=b["q"][i])[0]
        cont = (cia + np.sum(np.clip(np.nan_to_num(td1), 0, 1e20), 2)) + ray
        ref = oracle.cirsrad_ck_thermal(ISPACE, K, TPRESS, TTEMP, WAVE, delg, b["PRESS"][i], b["TEMP"][i], b["amount"][i], cont,
                                        b["NLAYIN"], b["LAYINC"], b["SCALE"], b["EMTEMP"][i], -1.0)
        np.testing.assert_allclose(got[i], ref, rtol=1e-10)


@pytest.mark.parametrize("tag", ["normal", "para"])
def test_batched_model_with_cia_fused_dense_and_per_state(golden, tag):
    """jacobian_nemesis_batched with CIA as a source of the model: fused and dense continuum give the same bits, on a side
    torch stream too; every state's spectrum equals the one-state route with its own calc_tau_cia; a perturbed level costs a
    few rows, not all."""
    import torch
    import archnemesis_dist_amd as pkg
    from archnemesis_dist_amd import synthetic as syn, layering
    from archnemesis_dist_amd.jacobian import jacobian_nemesis_batched, perturbed_states
    from archnemesis_dist_amd.profile_state import ContinuousProfileState, BatchedCKThermalModel
    NPRO, NLAY = 20, 16
    WAVE = grid(0)
    pr = syn.synth_profiles(NPRO, NVMR, seed=5, p_bottom_bar=5.0, p_top_bar=1.0e-5)
    st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("VMR", 1)])       # T and He: He reaches CIA alone
    names = ("CIA_WAVEN", "CIA_TEMP", "CIA_FRAC", "NPARA", "K_CIA", "IPAIRG1", "IPAIRG2", "INORMALT", "INORMAL", "INORMALD")
    tabs = cia_tables(golden, tag)
    PARAH2 = np.linspace(0.26, 0.48, NPRO) if tag == "para" else None
    eng = pkg.AnsfmEngine(0)
    try:
        eng.upload_ktable(*ktable(WAVE))
        model = BatchedCKThermalModel(eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], [2, 3, 4, 5],
                                      layering_args=dict(NLAY=NLAY, LAYINT=1, NINT=101),
                                      geometry=dict(pointing=layering.NADIR, EMISS_ANG=25.0, ANGLE=25.0), IRAY=4, PARAH2=PARAH2,
                                      cia=dict(zip(names, tabs)))
        assert model.fused_continuum is True
        YN, KK = jacobian_nemesis_batched(model)
        rows, total = model.last_rows
        model.fused_continuum = False
        YN_d, KK_d = jacobian_nemesis_batched(model)
        assert np.array_equal(YN, YN_d) and np.array_equal(KK, KK_d)
        model.fused_continuum = True
        side = torch.cuda.Stream(device=model.torch_device())
        with torch.cuda.stream(side):
            YN_s, KK_s = jacobian_nemesis_batched(model)
        assert np.array_equal(YN, YN_s) and np.array_equal(KK, KK_s)
        assert total == (st.NX + 1) * NLAY and rows < total // 3
        with pytest.raises(NotImplementedError):
            model.jacobian_analytic()
        # every state on its own
        st.calc_DSTEP()
        X = np.ascontiguousarray(perturbed_states(st.XN, st.DSTEP).T)
        Y = model.spectra_batch(X).cpu().numpy()
        assert np.array_equal(Y[0], YN)
        lay = model.layers(X)
        path = lay["path"]
        for i in range(X.shape[0]):
            cia = eng.calc_tau_cia(0, WAVE, *tabs, pr["ID"], pr["ISO"], lay["PP"][i], lay["PRESS"][i], lay["TEMP"][i], lay["FRAC"][i],
                                   lay["TOTAM"][i], lay["DELH"][i], with_grad=False)
            ray = eng.calc_tau_rayleigh(4, 0, WAVE, lay["TOTAM"][i], ID=pr["ID"], ISO=pr["ISO"], VMR=lay["VMRLAY"][i])[0]
            spec = eng.cirsrad_ck_thermal(0, lay["PRESS"][i:i + 1], lay["TEMP"][i:i + 1], lay["amount"][i:i + 1], (cia + ray)[None],
                                          path.NLAYIN, path.LAYINC, path.SCALE, path.EMTEMP[i:i + 1], np.array([-1.0]))
            np.testing.assert_allclose(Y[i], spec[0].reshape(-1), rtol=1e-10)
    finally:
        eng.close()


def test_batched_model_with_cia_and_aerosols_fused_dense_and_host_layers(golden):
    """CIA and two aerosol populations as sources of the model: the same (YN, KK) bits from the fused entry, from the dense
    continuum and from the layers through host arrays; the aerosols change the spectrum."""
    import archnemesis_dist_amd as pkg
    from archnemesis_dist_amd import synthetic as syn
    from archnemesis_dist_amd.jacobian import jacobian_nemesis_batched
    from archnemesis_dist_amd.profile_state import ContinuousProfileState, BatchedCKThermalModel
    NPRO, NLAY = 20, 16
    WAVE = grid(0)
    pr = syn.synth_profiles(NPRO, NVMR, seed=5, p_bottom_bar=5.0, p_top_bar=1.0e-5)
    st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T"])
    names = ("CIA_WAVEN", "CIA_TEMP", "CIA_FRAC", "NPARA", "K_CIA", "IPAIRG1", "IPAIRG2", "INORMALT", "INORMAL", "INORMALD")
    SWAVE, KEXT, KSCA = dust_table(WAVE, 2)
    DUST = 1.0e3 * np.exp(-np.linspace(0.0, 4.0, NPRO))[:, None] * np.array([1.0, 0.3])[None]
    eng = pkg.AnsfmEngine(0)
    try:
        eng.upload_ktable(*ktable(WAVE))
        mk = lambda dust: BatchedCKThermalModel(eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], [2, 3, 4, 5],
                                                layering_args=dict(NLAY=NLAY, LAYINT=1, NINT=101), IRAY=1,
                                                cia=dict(zip(names, cia_tables(golden, "normal"))), dust=dust)
        model = mk(dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA, DUST=DUST))
        YN, KK = jacobian_nemesis_batched(model)
        rows, total = model.last_rows
        assert total == (st.NX + 1) * NLAY and rows < total // 3
        model.fused_continuum = False
        YN_d, KK_d = jacobian_nemesis_batched(model)
        assert np.array_equal(YN, YN_d) and np.array_equal(KK, KK_d)
        model.device_layers = False
        YN_h, KK_h = jacobian_nemesis_batched(model)
        assert np.array_equal(YN, YN_h) and np.array_equal(KK, KK_h)
        YN_0, _ = jacobian_nemesis_batched(mk(None))
        assert not np.array_equal(YN, YN_0)
    finally:
        eng.close()


def test_refusals(golden):
    import archnemesis_dist_amd as pkg
    eng = pkg.AnsfmEngine(0)
    try:
        WAVE, b = grid(0), batch(golden, 0)
        tabs = cia_tables(golden, "normal")
        eng.upload_ktable(*ktable(WAVE))
        with pytest.raises(ValueError):                       # use_cia before upload_cia
            fused(eng, b, 0, 0, 0)
        eng.upload_cia(0, WAVE, *tabs, b["ID"], b["ISO"])
        assert fused(eng, b, 0, 0, 0).shape == (N, W, 1)
        eng.upload_ktable(*ktable(WAVE))                      # a new table clears the sources
        with pytest.raises(ValueError):
            fused(eng, b, 0, 0, 0)
        SWAVE, KEXT, KSCA = dust_table(WAVE, 8)
        with pytest.raises(NotImplementedError):
            eng.upload_dust(SWAVE, KEXT, KSCA)
        para = list(cia_tables(golden, "para"))
        para[2] = para[2][:-1]                                # CIA_FRAC shorter than NPARA
        with pytest.raises(NotImplementedError):
            eng.upload_cia(0, WAVE, *para, b["ID"], b["ISO"])
    finally:
        eng.close()
