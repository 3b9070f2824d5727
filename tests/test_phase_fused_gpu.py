"""The two batch entries that form the aerosol phase function on the device from the resident source (ansfm_upload_phase):
ansfm_cirsrad_ck_singlescatt_batch_src against ansfm_cirsrad_ck_singlescatt_batch_cont fed with phase_fn put together from
ansfm_phase_from_source / ansfm_calc_phase_ray, and ansfm_cirsrad_ck_scatter_batch_src against
ansfm_cirsrad_ck_scatter_batch_cont fed with the array read back (ansfm_phasarr_from_source) -- every comparison is
np.array_equal.  One anchor against something that is not this code: the single-scattering `_src` result against the dense
entry fed with NumPy arrays built from the reference's own phase function (tests/golden/phase.npz, `mie-paths`: the tabulated
mode is exact, so the whole chain is).  Then the refusals and the model classes with phase_source=.

The states, tables and sources are those of tests/singlescatt_cont_cases.py (W = 70, n = 8, NDUST = 2) and of
tests/test_scatter_cont_gpu.py (a small case of its builder)."""
import os

import numpy as np
import pytest

import phase_cases as pc
import singlescatt_cases as sc
import singlescatt_cont_cases as cc
import test_scatter_cont_gpu as ms

pytestmark = pytest.mark.gpu

THETA41 = pc.THETA41


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "tau_cia.npz"))


@pytest.fixture(scope="module")
def phase_golden(golden_dir):
    return pc.load_golden(os.path.join(golden_dir, "phase.npz"))


def phase_tables(imie, WAVE, ND, seed=11, SWAVE=None):
    """(imie, SWAVE, THETA_TAB, tab) of ND populations on SWAVE (None: an aerosol grid of 6 points around WAVE)"""
    rng = np.random.default_rng(seed + imie)
    SWAVE = np.linspace(WAVE.min() * 0.95, WAVE.max() * 1.05, 6) if SWAVE is None else SWAVE
    nws = len(SWAVE)
    if imie == 0:
        return 0, SWAVE, None, pc._hg_tab(rng, nws, ND)
    if imie == 1:
        return 1, SWAVE, THETA41, pc._mie_tab(rng, nws, THETA41, ND)
    return 2, SWAVE, None, pc._lp_tab(rng, nws, 12, ND)


def with_paths(c, paths):
    """the case with the paths `paths` of its two (a path may repeat): P = len(paths)"""
    base = dict(c["base"])
    for k in ("LAYINC", "BRDF"):
        base[k] = np.ascontiguousarray(base[k][:, paths])
    for k in ("NLAYIN", "sol", "emi"):
        base[k] = np.ascontiguousarray(base[k][paths])
    return dict(c, base=base, SCALE=np.ascontiguousarray(c["SCALE"][:, :, paths]), EMTEMP=np.ascontiguousarray(c["EMTEMP"][:, :, paths]))


def ss_src(eng, c, alpha, sel=slice(None)):
    b = c["b"]
    on = c["cia"] is not None
    return eng.cirsrad_ck_singlescatt_batch_src(c["ISPACE"], b["PRESS"][sel], b["TEMP"][sel], b["amount"][sel], b["q"][sel] if on else None,
                                                b["FRAC"][sel] if on else None, b["TOTAM"][sel], b["DELH"][sel] if on else None,
                                                b["CONT"][sel] if c["NDUST"] else None, c["IRAY"], None, alpha, *cc.rt_tail(c, sel),
                                                xfac=c["base"]["xfac"])


def phase_fn_of_source(eng, alpha):
    return np.ascontiguousarray(np.concatenate([eng.phase_from_source(alpha), np.broadcast_to(
        eng.calc_phase_ray(alpha)[None, :, None], (eng.ktable_info()[0][0], len(alpha), 1))], axis=2))


# ---- 1. single scattering ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("imie,ISPACE,paths", [(0, 0, [0, 1]), (1, 0, [0, 1]), (2, 0, [0, 1]), (1, 1, [0, 1]), (0, 0, [1]), (1, 0, [0, 1, 0])])
def test_singlescatt_src_equals_cont_fed_from_the_source(eng, golden, imie, ISPACE, paths):
    c = with_paths(cc.case(golden, ISPACE=ISPACE), paths)
    cc.upload(eng, c)
    eng.upload_phase(*phase_tables(imie, c["t"]["WAVE"], c["NDUST"]))
    alpha = np.array([147.3, 12.5, 90.0])[:len(paths)]
    c["phase_fn"] = phase_fn_of_source(eng, alpha)
    assert c["phase_fn"].shape == (c["W"], len(paths), 3) and np.all(np.isfinite(c["phase_fn"])) and np.all(c["phase_fn"][:, :, 2] > 0)
    try:
        for dedup in (True, False):
            eng.set_layer_dedup(dedup)
            ref = cc.fused(eng, c)
            rows = eng.last_layer_rows()
            got = ss_src(eng, c, alpha)
            assert got.shape == (c["n"], c["W"], len(paths)) and np.array_equal(got, ref)
            assert eng.last_layer_rows() == rows
        eng.set_layer_dedup(True)
        assert np.array_equal(ss_src(eng, c, alpha, sel=slice(2, 3)), ref[2:3])       # one state
    finally:
        eng.set_layer_dedup(True)
    assert not np.array_equal(ref[:, :, 0], ss_src(eng, c, alpha + 5.0)[:, :, 0])    # the angle reaches the spectrum


def test_singlescatt_src_against_the_reference_phase_function(eng, golden, phase_golden):
    """the anchor: the dense entry on NumPy arrays built from the reference's calc_phase (IRAY 0: the Rayleigh column of
    phase_fn multiplies TAURAY = 0 and adds an exact zero)"""
    from test_continuum_fused_gpu import dust_table
    d = phase_golden["mie-paths"]
    W, ND = d["wave"].shape[0], d["tab"].shape[2]
    c = cc.case(golden, cia=False, NDUST=ND, IRAY=0, W=W)
    c["t"]["WAVE"] = d["wave"].copy()
    c["dust"] = dict(zip(("SWAVE", "KEXT", "KSCA"), dust_table(d["wave"], ND)))
    c = with_paths(c, [0, 1, 1, 0])
    alpha = d["theta"]
    c["phase_fn"] = np.ascontiguousarray(np.concatenate([d["ref"], np.broadcast_to(
        pc.calc_phase_ray_np(alpha)[None, :, None], (W, 4, 1))], axis=2))
    cc.upload(eng, c)
    eng.upload_phase(1, d["swave"], d["ttab"], d["tab"])
    dense = cc.dense_batch(eng, c, cc.dense_arrays(eng, c))
    got = ss_src(eng, c, alpha)
    assert dense.shape == (c["n"], W, 4) and np.all(np.isfinite(dense)) and np.all(dense > 0)
    assert np.array_equal(got, dense)


# ---- 2. multiple scattering ---------------------------------------------------------------------------------------------------
def ms_src(eng, c, theta, imie, sel=slice(None), **over):
    b = c["b"]
    kw = dict(ws=None, CONT=b["CONT"][sel])
    kw.update(over)
    return eng.cirsrad_ck_scatter_batch_src(c["ISPACE"], b["PRESS"][sel], b["TEMP"][sel], b["amount"][sel], b["q"][sel], b["FRAC"][sel],
                                            b["TOTAM"][sel], b["DELH"][sel], kw["CONT"], c["IRAY"], None, theta,
                                            *ms.tail(c, sel=sel)[:-1], imie, wave_slice=kw["ws"])


def ms_cont(eng, c, phasarr, imie, sel=slice(None)):
    b = c["b"]
    return eng.cirsrad_ck_scatter_batch_cont(c["ISPACE"], b["PRESS"][sel], b["TEMP"][sel], b["amount"][sel], b["q"][sel], b["FRAC"][sel],
                                             b["TOTAM"][sel], b["DELH"][sel], b["CONT"][sel], c["IRAY"], None, phasarr,
                                             *ms.tail(c, sel=sel)[:-1], imie)


@pytest.mark.parametrize("NMU,NF", [(5, 2), (16, 3)])           # lane kernel, matrix-core chains
@pytest.mark.parametrize("imie,nth", [(0, 3), (0, 41), (1, 3), (1, 41)])
def test_scatter_src_equals_cont_fed_with_the_array(eng, golden, monkeypatch, imie, nth, NMU, NF):
    c = ms.case(golden, "normal", 0, 1, 2, NMU, NF, nW=70, n=3)
    ms.upload(eng, c)
    src = phase_tables(imie, c["z"]["WAVE"], 2)
    theta = THETA41 if nth == 41 else np.array([0.0, 90.0, 180.0])
    if imie == 1 and nth == 3:
        src = (1, src[1], theta, np.ascontiguousarray(src[3][:, [0, 20, 40]]))
    eng.upload_phase(*src)
    phasarr = eng.phasarr_from_source(theta)
    assert phasarr.shape == (2, 70, 2, nth)
    assert np.array_equal(phasarr[0, 0, 1], np.cos(theta * np.pi / 180)[::-1])
    if imie == 0:
        assert np.array_equal(phasarr[:, :, 0, :3], np.transpose(pc.hg_on_grid(src[1], src[3], c["z"]["WAVE"]), (1, 2, 0)))
    else:
        assert np.array_equal(phasarr[:, :, 0, ::-1], np.transpose(eng.phase_from_source(theta), (2, 0, 1)))
    ref = ms_cont(eng, c, phasarr, imie)
    assert ref.shape == (3, 70, 2) and np.all(np.isfinite(ref))
    got = ms_src(eng, c, theta, imie)
    assert np.array_equal(got, ref)
    assert eng.last_scatter_cache()[0] > 0
    monkeypatch.setenv("ANSFM_MS_LAYER_CACHE", "0")             # model by model
    assert np.array_equal(ms_src(eng, c, theta, imie), ref)
    assert eng.last_scatter_cache()[0] == 0


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_context_goes_on(eng, golden):
    c = cc.case(golden)
    cc.upload(eng, c)                                           # a new table: no phase source
    alpha = np.array([30.0, 120.0])
    with pytest.raises(ValueError, match="no phase-function source"):
        ss_src(eng, c, alpha)
    eng.upload_phase(*phase_tables(1, c["t"]["WAVE"], 3))
    with pytest.raises(ValueError, match="the phase-function source has 3 populations"):
        ss_src(eng, c, alpha)
    eng.upload_phase(*phase_tables(1, c["t"]["WAVE"], 2))
    with pytest.raises(ValueError, match="outside the tabulated angles"):
        ss_src(eng, c, np.array([30.0, 181.0]))
    with pytest.raises(ValueError):
        cc.fused(eng, c, phase_fn=None)                         # the existing entry still refuses a missing phase_fn
    c["phase_fn"] = phase_fn_of_source(eng, alpha)
    assert np.array_equal(ss_src(eng, c, alpha), cc.fused(eng, c))

    m = ms.case(golden, "normal", 0, 1, 2, 5, 2, nW=70, n=3)
    ms.upload(eng, m)
    with pytest.raises(ValueError, match="no phase-function source"):
        ms_src(eng, m, THETA41, 1)
    eng.upload_phase(*phase_tables(1, m["z"]["WAVE"], 3))
    with pytest.raises(ValueError, match="the phase-function source has 3 populations"):
        ms_src(eng, m, THETA41, 1)
    eng.upload_phase(*phase_tables(1, m["z"]["WAVE"], 2))
    with pytest.raises(ValueError, match="imie"):
        ms_src(eng, m, THETA41, 0)
    with pytest.raises(ValueError, match="ascending"):
        ms_src(eng, m, THETA41[::-1], 1)
    with pytest.raises(NotImplementedError, match="whole axis"):
        ms_src(eng, m, THETA41, 1, ws=(0, 140))
    with pytest.raises(NotImplementedError, match="whole axis"):
        ms_src(eng, m, THETA41, 1, ws=(5, 70))
    with pytest.raises(ValueError):
        ms.fused(eng, m, phasarr=None, CONT=m["b"]["CONT"])     # the existing entry still refuses a missing phasarr
    assert np.array_equal(ms_src(eng, m, THETA41, 1), ms_cont(eng, m, eng.phasarr_from_source(THETA41), 1))


# ---- 4. the model classes ------------------------------------------------------------------------------------------------------
def test_models_with_a_phase_source(golden):
    import archnemesis_dist_amd as pkg
    from archnemesis_dist_amd import synthetic as syn
    from archnemesis_dist_amd.jacobian import perturbed_states
    from archnemesis_dist_amd.profile_state import ContinuousProfileState
    from archnemesis_dist_amd.scatter_state import BatchedCKScatterModel, BatchedCKSingleScatterModel
    from test_continuum_fused_gpu import cia_tables, dust_table
    from test_gpu_parity import _scatter_inputs
    NPRO, NLAY, W = 10, 12, 70
    rng = np.random.default_rng(78)
    pr = syn.synth_profiles(NPRO, cc.NVMR, seed=5, p_bottom_bar=5.0, p_top_bar=1.0e-5)
    DUST = 1.0e3 * np.exp(-np.linspace(0.0, 4.0, NPRO))[:, None] * np.array([1.0, 0.3])[None]
    st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("DUST", 0)], DUST=DUST)
    st.calc_DSTEP()
    X = np.ascontiguousarray(perturbed_states(st.XN, st.DSTEP).T)[:4]
    cia = dict(zip(cc.CIA_NAMES, cia_tables(golden, "normal")))
    la = dict(NLAY=NLAY, LAYINT=1, NINT=101)
    eng = pkg.AnsfmEngine(0)
    try:
        # single scattering
        t = sc.synthetic_table("sorted", W, cc.G, 4)
        t["WAVE"] = cc.grid(0, W)
        sc.upload(eng, t)
        SWAVE, KEXT, KSCA = dust_table(t["WAVE"], 2)
        _, _, TT, tab = phase_tables(1, t["WAVE"], 2, SWAVE=SWAVE)     # the models upload it on the aerosol grid
        args = (eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], [2, 3, 4, 5])
        kw = dict(layering_args=la, geometry=dict(ANGLE=20.0, EMISS_ANG=20.0), IRAY=1, cia=cia, dust=dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA),
                  BRDF=rng.uniform(0.02, 0.15, (W, 1)), TSURF=150.0, emissivity=rng.uniform(0.7, 1.0, W))
        solar = 10.0 ** rng.uniform(-8, -7, W)
        model = BatchedCKSingleScatterModel(*args, None, [30.0], [20.0], solar, phase_source=(1, TT, tab), AZI_ANG=[45.0], **kw)
        Y = model.spectra_batch(X).cpu().numpy()
        assert Y.shape == (4, W) and np.all(np.isfinite(Y)) and not np.array_equal(Y[0], Y[1])
        alpha = eng.scattering_angle_deg([30.0], [20.0], [45.0])
        twin = BatchedCKSingleScatterModel(*args, phase_fn_of_source(eng, alpha), [30.0], [20.0], solar, **kw)
        twin._sources_on = True
        assert np.array_equal(twin.spectra_batch(X).cpu().numpy(), Y)
        with pytest.raises(ValueError):
            BatchedCKSingleScatterModel(*args, None, [30.0], [20.0], solar, phase_source=(1, TT, tab), **kw)      # no AZI_ANG
        with pytest.raises(ValueError):
            BatchedCKSingleScatterModel(*args, np.ones((W, 1, 3)), [30.0], [20.0], solar, phase_source=(1, TT, tab), AZI_ANG=[45.0], **kw)
        # multiple scattering
        NMU, NF = 5, 2
        z = _scatter_inputs(rng, W, ms.G, NLAY, 4, NMU, NF, 2, 1, 1, 1)
        z["WAVE"] = t["WAVE"]
        eng.upload_ktable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"], z["DELG"])
        geo = (z["MU"], z["WT"], NF, 101, ms.SOL, ms.EMI[False], ms.AZI, z["solar"])
        kw = dict(layering_args=la, IRAY=1, IMIE=1, cia=cia, dust=dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA), LOWBC=1, brdf_matrix=z["brdf"])
        model = BatchedCKScatterModel(*args, None, *geo, phase_source=(1, TT, tab), **kw)
        Y = model.spectra_batch(X).cpu().numpy()
        assert Y.shape == (4, 2 * W) and np.all(np.isfinite(Y)) and not np.array_equal(Y[0], Y[1])
        twin = BatchedCKScatterModel(*args, eng.phasarr_from_source(TT), *geo, **kw)
        twin._sources_on = True
        assert np.array_equal(twin.spectra_batch(X).cpu().numpy(), Y)
        with pytest.raises(NotImplementedError):
            model.spectra_batch(X, wave_slice=(0, 2 * W))
        with pytest.raises(ValueError):
            BatchedCKScatterModel(*args, None, *geo, phase_source=(0, TT, tab), **kw)       # IMIE = 1 with a Henyey-Greenstein source
    finally:
        eng.close()
