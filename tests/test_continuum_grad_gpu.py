"""The continuum gradients of a thermal CIRSrad(return_grad=True) call formed on the device from the resident CIA and aerosol
sources and the Rayleigh parametrisations (k_dtau_cont_rows, ansfm_cirsradg_ck_thermal_cont(_dev)): bit identity with the route
through calc_tau_cia(with_grad) / calc_tau_dust / calc_tau_rayleigh, a host-assembled dTAUCON and cirsradg_ck_thermal; the
oracle; central differences through the forward fused entry; BatchedCKThermalModel.jacobian_analytic(sources=True); refusals."""
import ctypes as C

import numpy as np
import pytest

from test_continuum_fused_gpu import W, S, L, NVMR, N, batch, cia_tables, dust_table, fused, golden, grid, ktable, sources  # noqa: F401

pytestmark = pytest.mark.gpu

IGAS = np.arange(2, 2 + S, dtype=np.int32)         # the spectroscopic gases are columns 2 .. 5: NVMR - 2 = 4 is one of them
TSURF = 250.0
EMIS = np.linspace(0.85, 1.0, W)


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


def assemble(cia, dcia, dust4, ray, dray, TOTAM, NDUST):
    """taucont (W, L) = (TAUCIA + TAUDUST) + TAURAY and dTAUCON (W, NPAR, L) as calculate_layer_opacity puts them together
    (forward_model._ansfm_continuum); ray / dray None: no Rayleigh term"""
    NPAR = NVMR + 2 + NDUST
    cont = cia
    if NDUST:
        cont = cont + np.sum(np.clip(np.nan_to_num(dust4[0]), 0, 1e20), 2)
    if ray is not None:
        cont = cont + ray
    d = np.zeros((W, NPAR, L))
    d[:, 0:NVMR, :] += np.moveaxis(dcia[:, :, 0:NVMR], 2, 1) / np.asarray(TOTAM)[None, None, :]
    d[:, NVMR, :] += dcia[:, :, NVMR]
    if dray is not None:
        for i in range(NVMR):
            d[:, i, :] += dray[:, :]
    for i in range(NDUST):
        d[:, NVMR + 1 + i, :] += dust4[2][:, :, i]
    return cont, d


def host_route(eng, b, tabs, dust, ISPACE, WAVE, IRAY, NDUST, i, tsurf=TSURF, emis=EMIS):
    """state i: the continuum and its gradients by the array-level entries, assembled in NumPy, through cirsradg_ck_thermal"""
    cia, dcia = eng.calc_tau_cia(ISPACE, WAVE, *tabs, b["ID"], b["ISO"], b["PP"][i], b["PRESS"][i], b["TEMP"][i], b["FRAC"][i],
                                 b["TOTAM"][i], b["DELH"][i])
    dust4 = eng.calc_tau_dust(WAVE, *dust, b["CONT"][i]) if NDUST else None
    ray, dray = eng.calc_tau_rayleigh(IRAY, ISPACE, WAVE, b["TOTAM"][i], ID=b["ID"], ISO=b["ISO"], VMR=b["q"][i]) if IRAY else (None, None)
    cont, dcont = assemble(cia, dcia, dust4, ray, dray, b["TOTAM"][i], NDUST)
    out = eng.cirsradg_ck_thermal(ISPACE, b["PRESS"][i], b["TEMP"][i], b["amount"][i], cont, dcont, NVMR, NVMR + 2 + NDUST, IGAS,
                                  b["NLAYIN"], b["LAYINC"], b["SCALE"], b["EMTEMP"][i], tsurf, EMISSIVITY=emis)
    return out, dcont


def fused_grad(eng, b, ISPACE, IRAY, NDUST, sel, tsurf=TSURF, emis=EMIS, **kw):
    q = b["q"][sel]
    f4 = eng.rayleigh_f4(b["ID"], b["ISO"], q) if IRAY == 4 else None
    return eng.cirsradg_ck_thermal_cont(ISPACE, b["PRESS"][sel], b["TEMP"][sel], b["amount"][sel], q, b["FRAC"][sel], b["TOTAM"][sel],
                                        b["DELH"][sel], b["CONT"][sel] if NDUST else None, IRAY, f4, NVMR, NVMR + 2 + NDUST, IGAS,
                                        b["NLAYIN"], b["LAYINC"], b["SCALE"], b["EMTEMP"][sel], tsurf, EMISSIVITY=emis, **kw)


def fused_grad_dev(eng, b, ISPACE, IRAY, NDUST, sel):
    import torch
    dev = torch.device("cuda", eng.device)
    td = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    n = b["PRESS"][sel].shape[0]
    NPAR = NVMR + 2 + NDUST
    spec, dts = (torch.empty((n, W, 1), dtype=torch.float64, device=dev) for _ in range(2))
    dspec = torch.empty((n, W, NPAR, L, 1), dtype=torch.float64, device=dev)
    f4 = td(eng.rayleigh_f4(b["ID"], b["ISO"], b["q"][sel])) if IRAY == 4 else None
    torch.cuda.current_stream(dev).synchronize()
    eng.cirsradg_ck_thermal_cont_dev(ISPACE, n, L, td(b["PRESS"][sel]), td(b["TEMP"][sel]), td(b["amount"][sel]), td(b["q"][sel]),
                                     td(b["FRAC"][sel]), td(b["TOTAM"][sel]), td(b["DELH"][sel]), td(b["CONT"][sel]) if NDUST else None,
                                     IRAY, f4, NVMR, NPAR, IGAS, 1, L, td(b["NLAYIN"], torch.int32), td(b["LAYINC"], torch.int32),
                                     td(np.repeat(b["SCALE"][None], n, 0)), td(b["EMTEMP"][sel]), td(np.full(n, TSURF)), td(EMIS), None,
                                     spec, dspec, dts)
    eng.synchronize()
    return spec.cpu().numpy(), dspec.cpu().numpy(), dts.cpu().numpy()


@pytest.mark.parametrize("NDUST", [0, 2])
@pytest.mark.parametrize("IRAY", [0, 1, 4])
@pytest.mark.parametrize("ISPACE", [0, 1])
@pytest.mark.parametrize("tag", ["normal", "para"])
def test_fused_gradient_continuum_is_bit_identical_with_the_host_assembled_route(eng, golden, tag, ISPACE, IRAY, NDUST):
    """states 0, 1 (a temperature differs) and 2 (He alone differs) of `batch`, each as one model and as a batch of three;
    with aerosols, layer 1 has a negative population: clipped in the opacity, raw in the gradient"""
    tabs, WAVE, b = cia_tables(golden, tag), grid(ISPACE), batch(golden, NDUST)
    dust = sources(eng, tabs, b, ISPACE, WAVE, NDUST)
    refs = [host_route(eng, b, tabs, dust, ISPACE, WAVE, IRAY, NDUST, i) for i in range(3)]
    for i, ((spec, dspec, dts), dcont) in enumerate(refs):
        assert np.all(np.isfinite(spec)) and np.all(np.isfinite(dspec)) and spec.min() > 0.0
        # He through CIA; gas NVMR - 2 is no CIA partner: its slot has calc_tau_cia's temperature term alone (:4667 takes it
        # between the para-H2 brackets, so it is zero without a para axis), and the Rayleigh term
        assert np.any(dcont[:, 1, :] != 0.0) and np.any(dcont[:, NVMR - 2, :] != 0.0) == (tag == "para" or IRAY != 0)
        assert not np.any(dcont[:, NVMR, :]) and not np.any(dcont[:, -1, :])               # temperature and para-H2 slots
        if NDUST:
            assert b["CONT"][i, 1, NDUST - 1] < 0 and np.all(dcont[:, NVMR + NDUST, 1] > 0)
        got = fused_grad(eng, b, ISPACE, IRAY, NDUST, i)
        assert np.array_equal(got[0], spec), i
        assert np.array_equal(got[1], dspec), i
        assert np.array_equal(got[2], dts), i
    assert not np.array_equal(refs[1][0][1], refs[0][0][1]) and not np.array_equal(refs[2][0][1], refs[0][0][1])
    got = fused_grad(eng, b, ISPACE, IRAY, NDUST, slice(0, 3))
    for k in range(3):
        assert np.array_equal(got[k], np.stack([r[0][k] for r in refs])), k
    if (tag, ISPACE, IRAY, NDUST) == ("para", 1, 4, 2):
        got = fused_grad_dev(eng, b, ISPACE, IRAY, NDUST, slice(0, 3))
        for k in range(3):
            assert np.array_equal(got[k], np.stack([r[0][k] for r in refs])), k


@pytest.mark.parametrize("tag,ISPACE,IRAY", [("normal", 0, 1), ("para", 1, 4)])
def test_fused_gradient_continuum_against_the_oracle(eng, oracle, golden, tag, ISPACE, IRAY):
    """oracle.calc_tau_cia (with gradients) + calc_tau_dust + calc_tau_rayleigh, the same assembly, oracle.cirsradg_ck_thermal;
    the bounds of test_gpu_parity.py for cirsradg_ck_thermal against the oracle: rtol 1e-10 for SPECOUT and dTSURF, 1e-9 of each
    parameter's largest gradient for dSPECOUT"""
    NDUST = 2
    tabs, WAVE, b = cia_tables(golden, tag), grid(ISPACE), batch(golden, NDUST)
    dust = sources(eng, tabs, b, ISPACE, WAVE, NDUST)
    K, TPRESS, TTEMP, _, delg = ktable(WAVE)
    i = 1
    spec, dspec, dts = fused_grad(eng, b, ISPACE, IRAY, NDUST, i)
    cia, dcia = oracle.calc_tau_cia(ISPACE, WAVE, *tabs, b["ID"], b["ISO"], b["PP"][i], b["PRESS"][i], b["TEMP"][i], b["FRAC"][i],
                                    b["TOTAM"][i], b["DELH"][i])
    dust4 = oracle.calc_tau_dust(WAVE, *dust, b["CONT"][i])
    ray, dray = oracle.calc_tau_rayleigh(IRAY, ISPACE, WAVE, b["TOTAM"][i], ID=b["ID"], ISO=b["ISO"], VMR=b["q"][i])
    cont, dcont = assemble(cia, dcia, dust4, ray, dray, b["TOTAM"][i], NDUST)
    rs, rd, rt = oracle.cirsradg_ck_thermal(ISPACE, K, TPRESS, TTEMP, WAVE, delg, b["PRESS"][i], b["TEMP"][i], b["amount"][i], cont, dcont,
                                            NVMR, NVMR + 2 + NDUST, IGAS, b["NLAYIN"], b["LAYINC"], b["SCALE"], b["EMTEMP"][i], TSURF,
                                            EMISSIVITY=EMIS)
    np.testing.assert_allclose(spec, rs, rtol=1e-10)
    np.testing.assert_allclose(dts, rt, rtol=1e-10, atol=0)
    scale = np.abs(rd).max(axis=(0, 2, 3), keepdims=True) + 1e-300
    worst = np.max(np.abs(dspec - rd) / scale)
    print("dSPECOUT against the oracle, worst / parameter maximum:", worst)
    assert worst < 1e-9


def test_fused_gradient_continuum_agrees_with_central_differences(eng, golden):
    """Central differences through the forward fused entry (cirsrad_ck_thermal_cont_dev), step 1e-4 of the value, to 1e-5 of the
    column's maximum as in test_analytic_jacobian_agrees_with_finite_differences (the contract is 1e-4).  (a) He's mixing ratio in
    layer 4: He is not spectroscopic, so only CIA moves, at fixed TOTAM; the gas slots are per unit column: x TOTAM.  Without a
    Rayleigh term, whose cross section the reference adds to every gas slot although it does not depend on the mixing ratio.
    (b) the first aerosol population of layer 6.  Temperature and the clipped population of layer 1 are not differenced: there
    the reference's gradient is not the derivative."""
    NDUST, ISPACE = 2, 0
    tabs, WAVE, b = cia_tables(golden, "normal"), grid(ISPACE), batch(golden, NDUST)
    sources(eng, tabs, b, ISPACE, WAVE, NDUST)
    pos = {int(l): j for j, l in enumerate(b["LAYINC"][:, 0])}
    one = lambda a: a[0:1].copy()

    def central(IRAY, key, idx, h):
        bb = dict(b)
        bb[key] = np.concatenate([one(b[key]), one(b[key])])
        bb[key][(0,) + idx] += h; bb[key][(1,) + idx] -= h
        for k in ("PRESS", "TEMP", "amount", "q", "FRAC", "TOTAM", "DELH", "CONT", "EMTEMP"):
            if k != key:
                bb[k] = np.concatenate([one(b[k]), one(b[k])])
        y = fused(eng, bb, ISPACE, IRAY, NDUST, sel=slice(0, 2))
        return (y[0] - y[1]) / (2 * h)

    # (a)
    _, dspec, _ = fused_grad(eng, b, ISPACE, 0, NDUST, 0, tsurf=-1.0, emis=None)
    ana = dspec[:, 1, pos[4], :] * b["TOTAM"][0, 4]
    fd = central(0, "q", (4, 1), 1.0e-4 * b["q"][0, 4, 1])
    worst_a = np.max(np.abs(fd - ana)) / np.abs(ana).max()
    # (b)
    _, dspec, _ = fused_grad(eng, b, ISPACE, 1, NDUST, 0, tsurf=-1.0, emis=None)
    ana = dspec[:, NVMR + 1, pos[6], :]
    fd = central(1, "CONT", (6, 0), 1.0e-4 * b["CONT"][0, 6, 0])
    worst_b = np.max(np.abs(fd - ana)) / np.abs(ana).max()
    print("central differences: He in layer 4", worst_a, " CONT[6, 0]", worst_b)
    assert np.abs(ana).max() > 0 and worst_a < 1e-5 and worst_b < 1e-5, (worst_a, worst_b)


def test_model_analytic_jacobian_with_sources(golden):
    """The model of test_batched_model_with_cia_and_aerosols_fused_dense_and_host_layers with the blocks T and ln VMR(He), IRAY 1:
    jacobian_analytic(sources=True) gives the bits of the chain built here from its layers (host-assembled dTAUCON ->
    cirsradg_ck_thermal -> map2pro -> map2xvec); YN is row 0 of spectra_batch to rtol 1e-12, the bound of the analytic route
    against the batched one in test_jacobian_c3.py; the bare call still refuses.  He is no spectroscopic gas: its columns of KK
    come from the continuum alone -- non-zero here, zero in a model without sources and without a Rayleigh term (whose cross
    section the reference adds to every gas's slot)."""
    import archnemesis_dist_amd as pkg
    from archnemesis_dist_amd import synthetic as syn
    from archnemesis_dist_amd.profile_state import ContinuousProfileState, BatchedCKThermalModel
    NPRO, NLAY, NDUST = 20, 16, 2
    WAVE = grid(0)
    pr = syn.synth_profiles(NPRO, NVMR, seed=5, p_bottom_bar=5.0, p_top_bar=1.0e-5)
    st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("VMR", 1)])
    names = ("CIA_WAVEN", "CIA_TEMP", "CIA_FRAC", "NPARA", "K_CIA", "IPAIRG1", "IPAIRG2", "INORMALT", "INORMAL", "INORMALD")
    tabs = cia_tables(golden, "normal")
    SWAVE, KEXT, KSCA = dust_table(WAVE, NDUST)
    DUST = 1.0e3 * np.exp(-np.linspace(0.0, 4.0, NPRO))[:, None] * np.array([1.0, 0.3])[None]
    eng = pkg.AnsfmEngine(0)
    try:
        eng.upload_ktable(*ktable(WAVE))
        model = BatchedCKThermalModel(eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], [2, 3, 4, 5],
                                      layering_args=dict(NLAY=NLAY, LAYINT=1, NINT=101), IRAY=1, cia=dict(zip(names, tabs)),
                                      dust=dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA, DUST=DUST))
        with pytest.raises(NotImplementedError, match="sources=True"):
            model.jacobian_analytic()
        YN, KK = model.jacobian_analytic(sources=True)
        assert KK.shape == (W, st.NX) and np.all(np.isfinite(KK))
        assert np.all(np.any(KK[:, NPRO:] != 0.0, axis=0))
        y0 = model.spectra_batch(st.XN[None]).cpu().numpy()[0]
        np.testing.assert_allclose(YN, y0, rtol=1e-12)
        # the chain from the layers of that call
        from archnemesis_dist_amd import layering
        lay = model.last_analytic_layers
        path = layering.calc_path(model.RADIUS, model.BASEH, lay["DELH"], lay["TEMP"], float(st.H[-1]), **model.geo)
        amount = np.ascontiguousarray(lay["AMOUNT"][:, [2, 3, 4, 5]].T) * 1.0e-4
        NPAR = NVMR + 2 + NDUST
        cia, dcia = eng.calc_tau_cia(0, WAVE, *tabs, pr["ID"], pr["ISO"], lay["PP"], lay["PRESS"], lay["TEMP"], lay["FRAC"],
                                     lay["TOTAM"], lay["DELH"])
        dust4 = eng.calc_tau_dust(WAVE, SWAVE, KEXT, KSCA, lay["CONT"])
        ray, dray = eng.calc_tau_rayleigh(1, 0, WAVE, lay["TOTAM"])
        cont = (cia + np.sum(np.clip(np.nan_to_num(dust4[0]), 0, 1e20), 2)) + ray
        dcont = np.zeros((W, NPAR, NLAY))
        dcont[:, 0:NVMR, :] += np.moveaxis(dcia[:, :, 0:NVMR], 2, 1) / lay["TOTAM"][None, None, :]
        dcont[:, NVMR, :] += dcia[:, :, NVMR]
        for i in range(NVMR):
            dcont[:, i, :] += dray
        for i in range(NDUST):
            dcont[:, NVMR + 1 + i, :] += dust4[2][:, :, i]
        eng.set_gradient_gases([], temperature=True)              # as the model: He is the only gas named, and it is in no table
        try:
            spec, _, _ = eng.cirsradg_ck_thermal(0, lay["PRESS"], lay["TEMP"], amount, cont, dcont, NVMR, NPAR, IGAS, path.NLAYIN,
                                                 path.LAYINC, path.SCALE, path.EMTEMP, -1.0, gradients_on_device=True)
            eng.map2pro(None, W, NVMR, NDUST, NPRO, path.NPATH, path.NLAYIN, path.LAYINC, lay["DTE"], lay["DAM"], lay["DCO"],
                        to_host=False)
        finally:
            eng.set_gradient_gases(None)
        xmap = np.zeros((st.NX, NPAR, NPRO)); lev = np.arange(NPRO)
        xmap[lev, NVMR, lev] = 1.0
        xmap[NPRO + lev, 1, lev] = st.profiles(st.XN[None])[1][0][:, 1]        # d VMR / d ln VMR at exp(XN), as the model takes it
        kk = eng.map2xvec(None, W, NVMR, NDUST, NPRO, path.NPATH, st.NX, xmap).reshape(W * path.NPATH, st.NX)
        assert np.array_equal(YN, spec.reshape(-1)) and np.array_equal(KK, kk)
        # no sources, no Rayleigh term: nothing reaches He
        bare = BatchedCKThermalModel(eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], [2, 3, 4, 5],
                                     layering_args=dict(NLAY=NLAY, LAYINT=1, NINT=101), IRAY=0)
        _, KK0 = bare.jacobian_analytic()
        assert not np.any(KK0[:, NPRO:]) and np.any(KK0[:, :NPRO])
    finally:
        eng.close()


def test_refusals(golden):
    """ValueError / NotImplementedError before any kernel: every refused call has two models, and the layer count of the last
    recorded call stays that of one"""
    import archnemesis_dist_amd as pkg
    eng = pkg.AnsfmEngine(0)
    try:
        WAVE, b = grid(0), batch(golden, 2)
        tabs = cia_tables(golden, "normal")
        eng.upload_ktable(*ktable(WAVE))
        two = slice(0, 2)
        ray_only = lambda nvmr, sel=0: eng.cirsradg_ck_thermal_cont(
            0, b["PRESS"][sel], b["TEMP"][sel], b["amount"][sel], None, None, b["TOTAM"][sel], None, None, 1, None, nvmr, nvmr + 2, IGAS,
            b["NLAYIN"], b["LAYINC"], b["SCALE"], b["EMTEMP"][sel], TSURF, EMISSIVITY=EMIS)
        args = lambda q, cont, nvmr, npar: (0, b["PRESS"][two], b["TEMP"][two], b["amount"][two], q, b["FRAC"][two], b["TOTAM"][two],
                                            b["DELH"][two], cont, 0, None, nvmr, npar, IGAS, b["NLAYIN"], b["LAYINC"], b["SCALE"],
                                            b["EMTEMP"][two], TSURF)

        def unmoved():
            assert eng.last_layer_rows()[1] == L

        assert ray_only(46)[1].shape == (W, 48, L, 1)            # the largest NVMR: 48 slots; one model of L layers is recorded
        unmoved()
        with pytest.raises(NotImplementedError):                 # NVMR + 2 > 48
            ray_only(47, two)
        unmoved()
        with pytest.raises(ValueError, match="CIA"):             # use_cia before upload_cia
            fused_grad(eng, b, 0, 0, 0, two)
        with pytest.raises(ValueError, match="aerosol"):         # aerosols before upload_dust
            eng.cirsradg_ck_thermal_cont(*args(None, b["CONT"][two], NVMR, NVMR + 4))
        unmoved()
        eng.upload_cia(0, WAVE, *tabs, b["ID"], b["ISO"])
        eng.upload_dust(*dust_table(WAVE, 2))
        with pytest.raises(ValueError, match="NVMR"):            # not the NVMR of the CIA source
            eng.cirsradg_ck_thermal_cont(*args(b["q"][two][:, :, :NVMR - 1], None, NVMR - 1, NVMR + 1))
        with pytest.raises(ValueError, match="NPAR"):            # not NVMR + 2 + the NDUST of the aerosol source
            eng.cirsradg_ck_thermal_cont(*args(b["q"][two], b["CONT"][two], NVMR, NVMR + 2 + 3))
        with pytest.raises(ValueError, match="ISPACE"):          # CIA uploaded for the other ISPACE
            eng.cirsradg_ck_thermal_cont(1, *args(b["q"][two], None, NVMR, NVMR + 2)[1:])
        unmoved()
        # a pending shared gas gradient: refused, and cancelled -- the next plain gradient call does not consume it
        plain = lambda: eng.cirsradg_ck_thermal(0, b["PRESS"][0], b["TEMP"][0], b["amount"][0], None, None, NVMR, NVMR + 2, IGAS,
                                                b["NLAYIN"], b["LAYINC"], b["SCALE"], b["EMTEMP"][0], TSURF, EMISSIVITY=EMIS)
        before = plain()
        armed = eng.cirsradg_ck_thermal(0, b["PRESS"][0], b["TEMP"][0], b["amount"][0], None, None, NVMR, NVMR + 2, IGAS, b["NLAYIN"],
                                        b["LAYINC"], b["SCALE"], b["EMTEMP"][0], TSURF, EMISSIVITY=EMIS, dtau_every_gas=np.ones((W, L)))
        assert not np.array_equal(armed[1], before[1])
        dray = np.ones((W, L))
        assert eng._lib.ansfm_set_shared_gas_gradient(eng._ctx, L, dray.ctypes.data_as(C.c_void_p)) == 0
        with pytest.raises(ValueError, match="shared gas gradient"):
            fused_grad(eng, b, 0, 1, 2, two)
        unmoved()
        after = plain()
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        assert fused_grad(eng, b, 0, 1, 2, two)[1].shape == (2, W, NVMR + 4, L, 1)      # and the entry is usable again
        assert eng.last_layer_rows()[1] == 2 * L
    finally:
        eng.close()
