"""The forward merge kernel's instruction trims against the CPU oracle, at the suite's 1e-11:
  * the peeled last G - 1 steps of every merge (shrinking list pass) and the one-offset walk, for every instantiated
    list length with and without padding entries (G = 12 runs in the 16-entry instantiation), through the array-level
    k_overlap and through the fused CIRSrad forward model;
  * tables with boxed (non-positive) entries keep the box tests, all-positive ones are read without them -- the flag the
    upload leaves and the numbers of both paths;
  * the last bin closed by the very last element of the merged order, and left open by it."""
import os
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-11
G_SWEEP = [8, 10, 12, 16, 20, 32]


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


def _relmax(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def _sweep_k(rng, W, G, L, S):
    """Sorted k(g) in four kinds along the wavenumber axis: random; flat to 1e-9 (a merged spectrum that is non-decreasing
    only up to rounding: the reorder of merge_init); the low g-ordinates of one gas zero in some columns; one gas zero
    altogether in some (wavenumber, layer) cells (the skip rules)."""
    k = np.sort(10.0 ** rng.uniform(-25, -20, (W, G, L, S)), axis=1)
    q = W // 4
    g = np.arange(G, dtype=np.float64)[None, :, None, None]
    k[q:2 * q] = 10.0 ** rng.uniform(-24, -21, (q, 1, L, S)) * (1.0 + g * 1e-9 / G)
    ncut = rng.integers(1, max(2, G // 2), size=(q, 1, L))
    s0 = S // 2
    k[2 * q:3 * q, :, :, s0] = np.where(np.arange(G)[None, :, None] < ncut, 0.0, k[2 * q:3 * q, :, :, s0])
    k[3 * q:, :, 0, 0] = 0.0                       # first gas empty: the second is taken as is
    k[3 * q:, :, L - 1, S - 1] = 0.0               # last gas empty: the merged spectrum is kept
    return k


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("G", G_SWEEP)
def test_k_overlap_sweep_vs_oracle(eng, oracle, G, S, f32):
    from archnemesis_dist_amd import synthetic as syn
    rng = np.random.default_rng(7000 + 10 * G + S)
    W, L = 136, 3                                  # 136: two full tiles and one with pad lanes
    _, delg = syn.gauss_legendre_01(G, f32)
    k = _sweep_k(rng, W, G, L, S)
    amount = 10.0 ** rng.uniform(19, 22, (S, L))
    tau = eng.k_overlap(delg, k, amount)
    ref = oracle.k_overlap(delg, k, amount)
    print(f"k_overlap G={G} S={S} f32={f32}: max rel err {_relmax(tau, ref):.3e}")
    np.testing.assert_allclose(tau, ref, rtol=RTOL, atol=0)


def _cirsrad_case(W, G, S, L, NP, NT, seed, f32=True):
    from archnemesis_dist_amd import synthetic as syn
    _, delg = syn.gauss_legendre_01(G, as_float32=f32)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=seed)
    WAVE = 250.0 + 0.5 * np.arange(W)
    atm = syn.synth_atmosphere(L, S, seed=seed + 1)
    atm["amount"][0, S - 1, 1] = 0.0               # skip rules: a gas without column in one layer
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, emiss_ang=20.0)
    cont = syn.synth_continuum(W, L)
    EMTEMP = atm["lay_temp"][0][LAYINC[:, 0]][:, None]
    return dict(delg=delg, PRESS=PRESS, TEMP=TEMP, K=K, WAVE=WAVE, atm=atm, NLAYIN=NLAYIN, LAYINC=LAYINC, SCALE=SCALE,
                cont=cont, EMTEMP=EMTEMP, L=L)


def _run_cirsrad(eng, c, K):
    eng.upload_ktable(K, c["PRESS"], c["TEMP"], c["WAVE"], c["delg"])
    a = c["atm"]
    spec = eng.cirsrad_ck_thermal(0, a["lay_press_pa"][0], a["lay_temp"][0], a["amount"][0], c["cont"][0], c["NLAYIN"],
                                  c["LAYINC"], c["SCALE"], c["EMTEMP"], -1.0)
    return np.squeeze(spec), eng.get_taugas(c["L"], 0)


def _ref_cirsrad(oracle, c, K):
    a = c["atm"]
    ref, tg = oracle.cirsrad_ck_thermal(0, K, c["PRESS"], c["TEMP"], c["WAVE"], c["delg"], a["lay_press_pa"][0],
                                        a["lay_temp"][0], a["amount"][0], c["cont"][0], c["NLAYIN"], c["LAYINC"], c["SCALE"],
                                        c["EMTEMP"], -1.0, return_taugas=True)
    return np.squeeze(ref), tg


@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("G", G_SWEEP)
def test_cirsrad_thermal_sweep_vs_oracle(eng, oracle, G, S):
    """The fused forward model on an all-positive table (read without the box tests): gas opacities and spectrum."""
    c = _cirsrad_case(70, G, S, 5, 5, 4, seed=300 + G + S, f32=(G != 12))
    spec, tg = _run_cirsrad(eng, c, c["K"])
    assert eng.ktable_info()[1] and not eng.ktable_has_boxed()
    ref, rtg = _ref_cirsrad(oracle, c, c["K"])
    print(f"cirsrad G={G} S={S}: taugas max rel err {_relmax(tg, rtg):.3e}, spectrum {_relmax(spec, ref):.3e}")
    np.testing.assert_allclose(tg, rtg, rtol=RTOL, atol=0)
    np.testing.assert_allclose(spec, ref, rtol=RTOL, atol=0)


def test_boxed_tables_keep_the_box_tests(eng, oracle):
    """One zero entry, one gas zero throughout, and their all-positive twin: the flag of each, every result against the
    oracle, and the twin read with and without the box tests gives the same bits."""
    G, S = 20, 4
    c = _cirsrad_case(100, G, S, 6, 5, 4, seed=77)
    twin = c["K"]
    one = twin.copy()
    one[37, 0, 2, 1, 1] = 0.0                      # first g-ordinate: the column stays non-decreasing
    gas = twin.copy()
    gas[..., 2] = 0.0
    for name, K, boxed in (("single zero entry", one, True), ("a whole gas zero", gas, True), ("all positive", twin, False)):
        spec, tg = _run_cirsrad(eng, c, K)
        assert eng.ktable_info()[1], name
        assert eng.ktable_has_boxed() is boxed, name
        ref, rtg = _ref_cirsrad(oracle, c, K)
        print(f"{name}: taugas max rel err {_relmax(tg, rtg):.3e}, spectrum {_relmax(spec, ref):.3e}")
        np.testing.assert_allclose(tg, rtg, rtol=RTOL, atol=0, err_msg=name)
        np.testing.assert_allclose(spec, ref, rtol=RTOL, atol=0, err_msg=name)
    # the twin is still uploaded: the same call with the box tests kept
    old = os.environ.get("ANSFM_LOAD_BOXTESTS")
    os.environ["ANSFM_LOAD_BOXTESTS"] = "1"
    try:
        spec2, tg2 = _run_cirsrad(eng, c, twin)
    finally:
        if old is None:
            del os.environ["ANSFM_LOAD_BOXTESTS"]
        else:
            os.environ["ANSFM_LOAD_BOXTESTS"] = old
    assert np.array_equal(tg, tg2) and np.array_equal(spec, spec2)


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("G", [8, 16, 20, 32])
def test_last_bin_closed_or_open_by_the_last_element(eng, oracle, G, closed):
    """Weights that are exact in binary (1/G for G a power of two; multiples of 2^-10 for G = 20), so the running weight
    sum of the walk is exact: with sum(del_g) = 1 it reaches g_ord[G] = 1 at the very last element of the merged order,
    which closes the last bin in a peeled step; with the last weight one unit shorter the sum ends below 1 and the last
    bin stays open (rank()'s trailing branch)."""
    rng = np.random.default_rng(900 + G)
    unit = 2.0 ** -10
    n = np.full(G, 1024 // G, dtype=np.int64)
    n[:1024 - int(n.sum())] += 1                   # G = 20: four weights of 52 units, sixteen of 51
    if not closed:
        n[-1] -= 1
    delg = n * unit
    assert bool(delg.sum() == 1.0) is closed and float(np.sum(np.outer(delg, delg))) <= 1.0
    W, L, S = 70, 2, 3
    k = np.sort(10.0 ** rng.uniform(-25, -20, (W, G, L, S)), axis=1)
    amount = 10.0 ** rng.uniform(19, 22, (S, L))
    for dg in (delg, delg.astype(np.float32)):     # float64 and float32 weight products (both exact here)
        tau = eng.k_overlap(dg, k, amount)
        ref = oracle.k_overlap(dg, k, amount)
        print(f"last bin G={G} closed={closed} {dg.dtype}: max rel err {_relmax(tau, ref):.3e}")
        np.testing.assert_allclose(tau, ref, rtol=RTOL, atol=0)
