"""CIRSrad's scattering branches on line-by-line tables (ILBL = 2): the gas opacities through calc_klbl in the three scattering
entry points, and the doubling / adding at G = 1 in spectral windows (phase matrices and Hansen factors of a window of
wavenumbers at a time, the walk carried from window to window).  Fixture: tools/golden/gen_golden_c4_lbl.py."""
import os

import numpy as np
import pytest

FIXTURE = "c4_lbl_scatter"


def _load(golden_dir):
    return np.load(os.path.join(golden_dir, FIXTURE + ".npz"))


def _ss(z, key):
    """the single-scattering run's array: its own (ss_) where it differs from the multiple-scattering run's"""
    return z["ss_" + key] if "ss_" + key in z.files else z[key]


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


# ---- without the GPU ---------------------------------------------------------------------------------------------------------
def test_fixture_pinned_by_the_oracle(golden_dir, oracle):
    """The reference's TAUGAS and scloud11wave_core radiance of the fixture, restated by the oracle: calc_klbl times the
    vertical columns, and the core at one g-ordinate."""
    z = _load(golden_dir)
    assert int(z["ILBL"]) == 2 and z["TAUGAS"].shape[1] == 1
    for get in (lambda k_: z[k_], lambda k_: _ss(z, k_)):
        k = oracle.calc_klbl(z["K"], z["TPRESS"], z["TTEMP"], get("LAY_PRESS") / 101325.0, get("LAY_TEMP"))
        am = np.ascontiguousarray(get("LAY_AMOUNT")[:, z["IGAS"]].T) * 1.0e-4
        taugas = np.zeros(k.shape[:2])
        for s in range(k.shape[2]):
            taugas += k[:, :, s] * am[s]
        np.testing.assert_allclose(taugas, get("TAUGAS")[:, 0, :], rtol=1e-10, atol=0)
    tautot = z["TAUGAS"] + (z["TAUCIA"] + z["TAUDUST"] + z["TAURAY"])[:, None, :]       # :3989
    np.testing.assert_allclose(tautot, z["TAUTOT"], rtol=1e-14, atol=0)
    rad = oracle.scloud11wave_core(z["core_phasarr"], z["core_radg"], z["SOL_ANG"], z["EMISS_ANG"], z["core_solar"], z["AZI_ANG"],
                                   int(z["LOWBC"]), z["core_brdf"], z["MU"], z["WTMU"], int(z["NF"]), z["WAVE"], z["core_bnu"],
                                   z["TAUTOT"], z["TAURAY"], z["core_omegas"], int(z["NPHI"]), int(z["IRAY"]),
                                   int(z["IMIE"]), z["core_lfrac"])
    assert rad.shape == z["core_rad"].shape and rad.shape[1] == 1
    assert np.max(np.abs(rad - z["core_rad"])) / np.max(np.abs(z["core_rad"])) < 1e-10


class _State:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _fake_model(ilbl, imod):
    from archnemesis_dist_amd import forward_model as fm

    class Model(fm.CIRSradGPU):
        pass

    m = Model()
    m.SpectroscopyX = _State(NGAS=2, ILBL=ilbl, K=np.zeros((4, 1, 2, 2, 2)))
    m.AtmosphereX = _State(NVMR=3)
    m.ScatterX = _State(NDUST=1)
    m.PathX = _State(IMOD=np.array([imod]))
    return m


def test_scattering_branches_dispatch_lbl_tables_to_the_gpu():
    from archnemesis_dist_amd import forward_model as fm
    ms = fm.IMOD_MULTIPLE_SCATTERING | 8192             # PLANCK_FUNCTION_AT_BIN_CENTRE | MULTIPLE_SCATTERING (the fixture's)
    ss = fm.IMOD_SINGLE_SCATTERING_PLANE_PARALLEL | 8192
    for imod in (ms, ss):
        assert _fake_model(fm.ILBL_LBL_TABLES, imod)._ansfm_supported(False)
        assert not _fake_model(fm.ILBL_LBL_TABLES, imod)._ansfm_supported(True)      # no gradients there in the reference
        assert _fake_model(fm.ILBL_K_TABLES, imod)._ansfm_supported(False)
    assert not _fake_model(1, ms)._ansfm_supported(False)                             # runtime line-by-line stays on the CPU


# ---- on the MI355X -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lbl_scatter_reference_golden(eng, golden_dir):
    """The reference's CIRSrad, multiple scattering on LBL tables (fixture): TAUGAS, the radiance before the quadrature and
    SPECOUT, at the tolerances of the k-table golden."""
    z = _load(golden_dir)
    assert int(z["IMOD"][0]) & 256 and not int(z["IMOD"][0]) & 64
    eng.upload_lbltable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"])
    f_gas = np.ascontiguousarray(z["LAY_AMOUNT"][:, z["IGAS"]].T) * 1.0e-4
    out, spec_g = eng.cirsrad_ck_scatter(int(z["ISPACE"]), z["LAY_PRESS"], z["LAY_TEMP"], f_gas, z["TAUCIA"], z["TAUDUST"],
                                         z["TAURAY"], z["TAUSCAT"], z["core_phasarr"], z["core_lfrac"], z["core_radg"],
                                         z["SOL_ANG"], z["EMISS_ANG"], z["AZI_ANG"], z["core_solar"], int(z["LOWBC"]),
                                         z["core_brdf"], z["MU"], z["WTMU"], int(z["NF"]), int(z["NPHI"]), int(z["IRAY"]),
                                         int(z["IMIE"]), return_spec_g=True)
    rt = 2e-7 if z["TPRESS"].dtype == np.float32 else 1e-11
    taugas = eng.get_taugas(z["LAY_PRESS"].size, 0)
    assert taugas.shape == z["TAUGAS"].shape
    np.testing.assert_allclose(taugas, z["TAUGAS"], rtol=rt, atol=0)
    ref_g = np.transpose(z["core_rad"], (2, 1, 0))
    assert np.max(np.abs(spec_g - ref_g)) / np.max(np.abs(ref_g)) < max(1e-8, 10 * rt)
    assert np.max(np.abs(out - z["SPECOUT"]) / np.abs(z["SPECOUT"])) < max(1e-8, 10 * rt)


@pytest.mark.gpu
def test_lbl_singlescatt_reference_golden(eng, golden_dir):
    """The reference's CIRSrad, single scattering (plane parallel) on LBL tables (fixture, keys ss_)."""
    z = _load(golden_dir)
    assert int(_ss(z, "IMOD")[0]) & 1024 and int(_ss(z, "IFORM")) == 0
    eng.upload_lbltable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"])
    f_gas = np.ascontiguousarray(_ss(z, "LAY_AMOUNT")[:, z["IGAS"]].T) * 1.0e-4
    out = eng.cirsrad_ck_singlescatt(int(_ss(z, "ISPACE")), _ss(z, "LAY_PRESS"), _ss(z, "LAY_TEMP"), f_gas,
                                     _ss(z, "TAUCIA") + _ss(z, "TAUDUST") + _ss(z, "TAURAY"), _ss(z, "TAURAY") + _ss(z, "TAUSCAT"),
                                     _ss(z, "PHASE"), _ss(z, "NLAYIN"), _ss(z, "LAYINC"), _ss(z, "SCALE"), _ss(z, "EMTEMP"),
                                     float(_ss(z, "TSURF")), _ss(z, "EMISSIVITY"), _ss(z, "BRDF"), _ss(z, "SOLFLUX"), _ss(z, "SOL_ANG"),
                                     _ss(z, "EMISS_ANG"))
    rt = 2e-7 if z["TPRESS"].dtype == np.float32 else 1e-11
    np.testing.assert_allclose(eng.get_taugas(_ss(z, "LAY_PRESS").size, 0), _ss(z, "TAUGAS"), rtol=rt, atol=0)
    ref = _ss(z, "SPECOUT")
    assert out.shape == ref.shape and np.all(np.abs(ref) > 0)
    assert np.max(np.abs(out - ref) / np.abs(ref)) < max(1e-8, 10 * rt)


def _lbl_inputs(rng, W, L, S, NMU, NF, ncont, imie, iray, lowbc, wave0=600.0):
    """Seeded LBL table and the scattering inputs of ansfm_cirsrad_ck_scatter in the reference's layouts."""
    NP, NT = 6, 4
    PRESS = np.logspace(-5, 1, NP); TEMP = np.linspace(90.0, 300.0, NT)
    K = (10.0 ** rng.uniform(-25, -21, (W, 1, 1, S))) * PRESS[None, :, None, None] ** 0.15 * (TEMP[None, None, :, None] / 150.0) ** 0.8
    WAVE = wave0 + 0.01 * np.arange(W)
    lay_p = np.logspace(5.3, 1.5, L); lay_t = np.linspace(165.0, 110.0, L)
    amount = 10.0 ** rng.uniform(19.0, 21.0, (S, 1)) * (lay_p[None, :] / lay_p[0]) ** 0.9
    TAUCIA = 10.0 ** rng.uniform(-5, -2, (W, L)); TAURAY = (10.0 ** rng.uniform(-6, -3, (W, L))) * (1.0 if iray else 0.0)
    nc = ncont
    clscat = 10.0 ** rng.uniform(-5, -1.5, (W, L, nc))
    clscat[:, min(2, L - 1), :] = 0.0                                       # a layer without aerosol
    TAUSCAT = clscat.sum(axis=2)
    TAUDUST = TAUSCAT * rng.uniform(1.02, 1.5, (W, L)) if ncont else 10.0 ** rng.uniform(-5, -3, (W, L))
    lfrac = np.zeros((W, nc, L))
    pos = TAUSCAT > 0
    lfrac[:] = np.transpose(np.where(pos[:, :, None], clscat / np.where(pos, TAUSCAT, 1.0)[:, :, None], 0.0), (0, 2, 1))
    x, w = np.polynomial.legendre.leggauss(2 * NMU)
    MU = 0.5 * (x[NMU:] + 1.0); MU[-1] = 1.0; WT = w[NMU:] * 0.5
    THETA = np.linspace(0.0, 180.0, 41)
    PH = np.zeros((nc, W, 2, THETA.size))
    if imie == 0:                                                           # double Henyey-Greenstein parameters
        PH[:, :, 0, -1] = rng.uniform(0.6, 0.95, (nc, W)); PH[:, :, 0, -2] = rng.uniform(0.3, 0.8, (nc, W))
        PH[:, :, 0, -3] = rng.uniform(-0.5, -0.1, (nc, W))
    else:                                                                   # tabulated
        c = np.cos(np.deg2rad(THETA))
        gg = rng.uniform(0.2, 0.7, (nc, W, 1))
        PH[:, :, 0, :] = (1 - gg * gg) / (1 + gg * gg - 2 * gg * c) ** 1.5 / (4 * np.pi)
    PH[:, :, 1, :] = np.cos(THETA * np.pi / 180)
    phasarr = np.ascontiguousarray(PH[:, :, :, ::-1])
    c1, c2 = 1.1911e-12, 1.439
    radg = np.repeat((c1 * WAVE ** 3 / (np.exp(c2 * WAVE / lay_t[0]) - 1.0))[:, None], NMU, 1)
    solar = 10.0 ** rng.uniform(-9, -8, W)
    brdf = np.zeros((W, NMU, NMU, NF + 1))
    if lowbc:
        brdf[:, :, :, 0] = rng.uniform(0.05, 0.3, (W, 1, 1)) / np.pi
    return dict(K=K, TPRESS=PRESS, TTEMP=TEMP, WAVE=WAVE, lay_p=lay_p, lay_t=lay_t, amount=amount, TAUCIA=TAUCIA,
                TAUDUST=TAUDUST, TAURAY=TAURAY, TAUSCAT=TAUSCAT, lfrac=lfrac, phasarr=phasarr, radg=radg, solar=solar,
                brdf=brdf, MU=MU, WT=WT, ncont=ncont, iray=iray, imie=imie, lowbc=lowbc, NF=NF)


def _geometry(up):
    sol = np.array([30.0, 120.0]); emi = np.array([160.0, 130.0]) if up else np.array([20.0, 50.0]); azi = np.array([45.0, 0.0])
    return sol, emi, azi


def _scatter(eng, z, up, spec_g=False, **kw):
    sol, emi, azi = _geometry(up)
    ncont, iray = z["ncont"], z["iray"]
    return eng.cirsrad_ck_scatter(0, z["lay_p"], z["lay_t"], z["amount"], z["TAUCIA"], z["TAUDUST"], z["TAURAY"] if iray else None,
                                  z["TAUSCAT"], z["phasarr"] if ncont else None, z["lfrac"] if ncont else None, z["radg"], sol, emi,
                                  azi, z["solar"], z["lowbc"], z["brdf"], z["MU"], z["WT"], z["NF"], 101, iray, z["imie"],
                                  return_spec_g=spec_g, **kw)


def _lbl_oracle(oracle, z, up, w=slice(None)):
    """The reference's recipe on the oracle's restatements: calc_klbl times the columns (:3795-3817), TAUTOT (:3989),
    OMEGA / BB (:5099-5119), scloud11wave_core at one g-ordinate; wavenumbers w only."""
    sol, emi, azi = _geometry(up)
    k = oracle.calc_klbl(z["K"][w], z["TPRESS"], z["TTEMP"], z["lay_p"] / 101325.0, z["lay_t"])
    taugas = np.zeros(k.shape[:2])
    for s in range(k.shape[2]):
        taugas += k[:, :, s] * z["amount"][s]
    taugas = taugas[:, None, :]
    cia, dust, ray, sca = (z[n][w] for n in ("TAUCIA", "TAUDUST", "TAURAY", "TAUSCAT"))
    tautot = taugas + cia[:, None, :] + dust[:, None, :] + ray[:, None, :]
    omega = np.zeros_like(tautot)
    pos = tautot > 0
    omega[pos] = np.broadcast_to((ray + sca)[:, None, :], tautot.shape)[pos] / tautot[pos]
    c1, c2 = 1.1911e-12, 1.439
    wave = z["WAVE"][w]
    bnu = c1 * wave[:, None] ** 3 / (np.exp(c2 * wave[:, None] / z["lay_t"][None, :]) - 1.0)
    rad = oracle.scloud11wave_core(z["phasarr"][:, w], z["radg"][w], sol, emi,
                                   z["solar"][w], azi, z["lowbc"], z["brdf"][w], z["MU"], z["WT"], z["NF"], wave, bnu, tautot, ray,
                                   omega, 101, z["iray"], z["imie"], z["lfrac"][w])
    return np.transpose(rad, (2, 1, 0)), taugas


@pytest.mark.gpu
@pytest.mark.parametrize("NMU,NF,ncont,imie,iray,lowbc,up", [(5, 2, 2, 0, 1, 0, False), (5, 1, 1, 1, 1, 1, True),
                                                             (16, 3, 1, 1, 1, 1, False), (16, 2, 2, 0, 1, 0, True),
                                                             (8, 2, 1, 0, 1, 1, False), (12, 2, 1, 1, 1, 0, True),
                                                             (16, 2, 0, 0, 1, 1, True),     # no aerosol: Rayleigh, Lambert, look-up
                                                             (5, 2, 0, 0, 1, 1, True)])
def test_lbl_scatter_vs_oracle(eng, oracle, NMU, NF, ncont, imie, iray, lowbc, up):
    rng = np.random.default_rng(3100 + NMU + 7 * NF + 3 * ncont + imie + 11 * lowbc)
    W, L, S = 40, 7, 3
    z = _lbl_inputs(rng, W, L, S, NMU, NF, ncont, imie, iray, lowbc)
    eng.upload_lbltable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"])
    out, spec_g = _scatter(eng, z, up, spec_g=True)
    ref_g, taugas = _lbl_oracle(oracle, z, up)
    np.testing.assert_allclose(eng.get_taugas(L, 0), taugas, rtol=1e-11, atol=0)
    assert np.max(np.abs(spec_g - ref_g)) / np.max(np.abs(ref_g)) < 1e-8
    assert np.max(np.abs(out - ref_g[:, 0, :])) / np.max(np.abs(ref_g)) < 1e-8     # DELG = {1}


@pytest.mark.gpu
@pytest.mark.parametrize("NMU,NF,ncont,imie,lowbc,up", [(5, 2, 1, 0, 1, False), (16, 3, 2, 1, 0, True)])
def test_lbl_scatter_window_size_changes_no_bit(eng, monkeypatch, NMU, NF, ncont, imie, lowbc, up):
    """G = 1: the phase matrices and Hansen factors of a window of wavenumbers at a time, the walk continuing from the carry of
    the window before.  Every window size gives the same bits; a G > 1 k-table call ignores ANSFM_MS_WINDOW."""
    rng = np.random.default_rng(3300 + NMU)
    W, L, S = 1500, 12, 2
    z = _lbl_inputs(rng, W, L, S, NMU, NF, ncont, imie, 1, lowbc)
    eng.upload_lbltable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"])
    runs = {}
    for nwin in (W, 1000, 333, 64):
        monkeypatch.setenv("ANSFM_MS_WINDOW", str(nwin))
        runs[nwin] = _scatter(eng, z, up, spec_g=True)
        assert eng.last_scatter_windows() == (-(-W // nwin), nwin)
    monkeypatch.delenv("ANSFM_MS_WINDOW")
    default = _scatter(eng, z, up, spec_g=True)
    assert eng.last_scatter_windows() == (1, W)                     # W < 4096: one window by default
    for nwin, (out, spec_g) in runs.items():
        assert np.array_equal(spec_g, default[1]), nwin
        assert np.array_equal(out, default[0]), nwin
    # G > 1 (k-table): one window whatever the variable says
    from archnemesis_dist_amd import synthetic as syn
    Wk, G = 300, 4
    PRESS, TEMP, K = syn.synth_ktable(Wk, G, 6, 4, S, seed=5)
    _, delg = syn.gauss_legendre_01(G)
    zk = dict(z)
    for n in ("TAUCIA", "TAUDUST", "TAURAY", "TAUSCAT", "radg", "solar", "brdf"):
        zk[n] = z[n][:Wk]
    zk["phasarr"] = z["phasarr"][:, :Wk]; zk["lfrac"] = z["lfrac"][:Wk]
    eng.upload_ktable(K, PRESS, TEMP, z["WAVE"][:Wk], delg)
    ref = _scatter(eng, zk, up, spec_g=True)
    monkeypatch.setenv("ANSFM_MS_WINDOW", "64")
    got = _scatter(eng, zk, up, spec_g=True)
    assert eng.last_scatter_windows() == (1, Wk)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


@pytest.mark.gpu
@pytest.mark.parametrize("NMU,cache,env", [(5, True, ("ANSFM_MS_SLAB", "40")), (16, True, ("ANSFM_MS_SLAB", "50")),
                                           (16, True, None), (5, False, ("ANSFM_MS_WINDOW", "64")),
                                           (16, False, ("ANSFM_MS_WINDOW", "64"))])
def test_lbl_scatter_batch_equals_separate_calls(eng, monkeypatch, NMU, cache, env):
    """ansfm_cirsrad_ck_scatter_batch on an LBL table: the forward models of a numerical Jacobian, bit-identical to calls of
    their own -- with the layer cache (slabs of the spectral axis = windows, ANSFM_MS_SLAB) and model by model (the walk
    recomputed per model when several windows cover the axis)."""
    rng = np.random.default_rng(3500 + NMU + 2 * int(cache))
    W, L, S, NF = 200, 9, 2, 2
    z = _lbl_inputs(rng, W, L, S, NMU, NF, 1, 1, 1, 1)
    eng.upload_lbltable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"])
    n = 5
    rep = lambda a: np.repeat(np.asarray(a)[None], n, 0).copy()
    lp, lt, am = rep(z["lay_p"]), rep(z["lay_t"]), rep(z["amount"])
    cia, dust, ray, sca = rep(z["TAUCIA"]), rep(z["TAUDUST"]), rep(z["TAURAY"]), rep(z["TAUSCAT"])
    lf, rg = rep(z["lfrac"]), rep(z["radg"])
    lt[1, 4] *= 1.05                                   # a layer temperature
    am[2, 1, 6] *= 1.05                                # a gas amount
    sca[3, :, 3] *= 1.05; dust[3, :, 3] *= 1.05        # the aerosol of a layer
    lt[4] *= 1.01                                      # everything
    sol, emi, azi = _geometry(False)
    tail = (sol, emi, azi, z["solar"], 1, z["brdf"], z["MU"], z["WT"], NF, 101, 1, 1)
    ref = np.stack([eng.cirsrad_ck_scatter(0, lp[m], lt[m], am[m], cia[m], dust[m], ray[m], sca[m], z["phasarr"], lf[m], rg[m], *tail)
                    for m in range(n)])
    if env is not None:
        monkeypatch.setenv(*env)
    if not cache:
        eng.set_layer_dedup(False)
    try:
        got = eng.cirsrad_ck_scatter_batch(0, lp, lt, am, cia, dust, ray, sca, z["phasarr"], lf, rg, *tail)
    finally:
        eng.set_layer_dedup(True)
    assert np.array_equal(got, ref)
    nw, ww = eng.last_scatter_windows()
    if env is not None:
        assert nw > 1 and nw == -(-W // ww)
    if cache:
        hits, total = eng.last_scatter_cache()
        assert total == (n - 1) * L and hits == total - (1 + 1 + 1 + L)


@pytest.mark.gpu
def test_lbl_scatter_full_size_in_windows(eng, oracle):
    """2e5 wavenumbers x one g-ordinate x 100 layers, 16 streams, 9 Fourier orders, the C4 haze + Rayleigh: the call completes in
    several windows, each within the buffer budget, and its first 256 wavenumbers are the oracle's on those 256 alone (the
    walk carries history along the axis from its first wavenumber on)."""
    rng = np.random.default_rng(3700)
    W, L, S, NMU, NF = 200_000, 100, 2, 16, 8
    z = _lbl_inputs(rng, W, L, S, NMU, NF, 1, 1, 1, 0)
    # the C4 haze (tools/c4_run.py): a tabulated phase function of asymmetry 0.6, 36 Legendre moments
    TH = np.linspace(0.0, 180.0, 41); c = np.cos(np.deg2rad(TH))
    leg = np.polynomial.legendre.legval(c, 0.6 ** np.arange(36) * (2 * np.arange(36) + 1)) / (4 * np.pi)
    ph = np.zeros((1, W, 2, TH.size)); ph[0, :, 0, :] = leg[None, :]; ph[0, :, 1, :] = c[None, :]
    z["phasarr"] = np.ascontiguousarray(ph[:, :, :, ::-1])
    eng.upload_lbltable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"])
    out = _scatter(eng, z, False)
    nw, ww = eng.last_scatter_windows()
    ncomp = 2
    per_w = (2 * (NF + 1) + 1) * ncomp * NMU * NMU * 8                      # phase matrices + Hansen factors of one wavenumber
    assert nw > 1 and nw == -(-W // ww) and ww * per_w <= (2 << 30)
    assert out.shape == (W, 2) and np.all(np.isfinite(out))
    ref_g, _ = _lbl_oracle(oracle, z, False, slice(0, 256))
    assert np.max(np.abs(out[:256] - ref_g[:, 0, :])) / np.max(np.abs(ref_g)) < 1e-8
