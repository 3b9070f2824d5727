"""The forward merge kernel's list pass that ends at the insertion point (kMergeExit) and its per-lane choice of the row operand
(kMergeOrient) against the code without any trim (ANSFM_MERGE_LEGACY=1) bit for bit, and both against the CPU
oracle at the suite's 1e-11.  The inputs change along the wavenumber axis, so that one wave holds lanes of both orientations:
the four kinds of tests/test_merge_trim.py::_sweep_k (random; flat to 1e-9; low g-ordinates zero; a gas zero in some cells,
which makes the skip rules lane-divergent), every later gas 1e6 times the one before and the reverse, and every gas flat to
1e-9 -- there the merged spectrum need not be monotone (such a lane must keep its orientation) and keys tie, so the low key
bits decide the order.  Every instantiated list length with and without padding entries, float32 weights (the table path),
through the array-level k_overlap and through the fused CIRSrad forward model; fewer tiles than waves; a batch of models.
Every case asserts that the launch it compares reported both trims."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-11
G_SWEEP = [8, 10, 12, 16, 20, 32]
EXIT, ORIENT = 8, 16                               # bits of ansfm_last_merge_launch's trims


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


@contextmanager
def _legacy():
    old = os.environ.get("ANSFM_MERGE_LEGACY")
    os.environ["ANSFM_MERGE_LEGACY"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["ANSFM_MERGE_LEGACY"]
        else:
            os.environ["ANSFM_MERGE_LEGACY"] = old


def _check_launches(new_launch, old_launch):
    waves, trims = new_launch
    assert trims & EXIT and trims & ORIENT and trims & 1 and waves > 1, new_launch
    assert old_launch == (1, 0), old_launch


def _delg(G):
    from archnemesis_dist_amd import synthetic as syn
    _, delg = syn.gauss_legendre_01(G, as_float32=True)
    return delg.astype(np.float32)


def _relmax(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def _mixed_k(rng, W, G, L, S, positive=False):
    """Seven kinds along the wavenumber axis (W // 7 columns each, the first kind takes the rest), interleaved so that every
    64-lane tile holds several: 0 random; 1 flat to 1e-9, every gas; 2 the low g-ordinates of one gas zero; 3 one gas zero
    altogether in some cells; 4 gas s = 1e6^min(s, 3) times a random one (b dominates: rows from b); 5 the reverse (a
    dominates); 6 flat to 1e-9 with the gases decades apart.  positive: kinds 2 and 3 are random instead (no boxed entry)."""
    k = np.sort(10.0 ** rng.uniform(-25, -20, (W, G, L, S)), axis=1)
    kind = np.arange(W) % 7
    g = np.arange(G, dtype=np.float64)[None, :, None, None]
    s = np.arange(S)
    flat = lambda n: 10.0 ** rng.uniform(-24, -21, (n, 1, L, S)) * (1.0 + g * 1e-9 / G)
    k[kind == 1] = flat(int(np.sum(kind == 1)))
    if not positive:
        n2 = int(np.sum(kind == 2))
        ncut = rng.integers(1, max(2, G // 2), size=(n2, 1, L))
        s0 = S // 2
        k2 = k[kind == 2]
        k2[:, :, :, s0] = np.where(np.arange(G)[None, :, None] < ncut, 0.0, k2[:, :, :, s0])
        k[kind == 2] = k2
        k3 = k[kind == 3]
        k3[:, :, 0, 0] = 0.0
        k3[:, :, L - 1, S - 1] = 0.0
        k3[::2, :, L // 2, S // 2] = 0.0
        k[kind == 3] = k3
    k[kind == 4] *= 1e6 ** np.minimum(s, 3)
    k[kind == 5] *= 1e6 ** np.maximum(3 - s, 0)
    k[kind == 6] = flat(int(np.sum(kind == 6))) * 1e3 ** ((s * 5) % 4)
    return k


@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("G", G_SWEEP)
def test_k_overlap_exit_and_orientation(eng, oracle, G, S):
    rng = np.random.default_rng(6100 + 10 * G + S)
    W, L = 136, 3                                  # two full tiles and one with pad lanes
    delg = _delg(G)
    k = _mixed_k(rng, W, G, L, S)
    amount = 10.0 ** rng.uniform(19, 22, (S, L))
    new = eng.k_overlap(delg, k, amount)
    new_launch = eng.last_merge_launch()
    with _legacy():
        old = eng.k_overlap(delg, k, amount)
        old_launch = eng.last_merge_launch()
    _check_launches(new_launch, old_launch)
    ref = oracle.k_overlap(delg, k, amount)
    print(f"k_overlap G={G} S={S}: new vs oracle {_relmax(new, ref):.3e}, old vs oracle {_relmax(old, ref):.3e}, "
          f"bits equal {np.array_equal(new, old)}")
    assert np.array_equal(new, old)
    np.testing.assert_allclose(new, ref, rtol=RTOL, atol=0)
    np.testing.assert_allclose(old, ref, rtol=RTOL, atol=0)


def _cirsrad_case(rng, W, G, S, L, positive):
    from archnemesis_dist_amd import synthetic as syn
    NP, NT = 3, 2
    delg = _delg(G)
    PRESS, TEMP, _ = syn.synth_ktable(8, G, NP, NT, S, seed=5)
    K = np.ascontiguousarray(_mixed_k(rng, W, G, NP * NT, S, positive).reshape(W, G, NP, NT, S))
    WAVE = 250.0 + 0.5 * np.arange(W)
    atm = syn.synth_atmosphere(L, S, seed=11)
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, emiss_ang=20.0)
    cont = syn.synth_continuum(W, L)
    EMTEMP = atm["lay_temp"][0][LAYINC[:, 0]][:, None]
    return dict(delg=delg, PRESS=PRESS, TEMP=TEMP, K=K, WAVE=WAVE, atm=atm, NLAYIN=NLAYIN, LAYINC=LAYINC, SCALE=SCALE,
                cont=cont, EMTEMP=EMTEMP, L=L)


def _run_cirsrad(eng, c):
    a = c["atm"]
    spec = eng.cirsrad_ck_thermal(0, a["lay_press_pa"][0], a["lay_temp"][0], a["amount"][0], c["cont"][0], c["NLAYIN"],
                                  c["LAYINC"], c["SCALE"], c["EMTEMP"], -1.0)
    return np.squeeze(spec), eng.get_taugas(c["L"], 0)


@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("G", G_SWEEP)
def test_cirsrad_exit_and_orientation(eng, oracle, G, S):
    rng = np.random.default_rng(5100 + 10 * G + S)
    for positive in (True, False):                 # read without / with the box tests: two instantiations
        c = _cirsrad_case(rng, 136, G, S, 3, positive)
        eng.upload_ktable(c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"])
        assert eng.ktable_info()[1]                # monotone: the fast path
        assert eng.ktable_has_boxed() is (not positive)
        spec, tg = _run_cirsrad(eng, c)
        new_launch = eng.last_merge_launch()
        with _legacy():
            spec0, tg0 = _run_cirsrad(eng, c)
            old_launch = eng.last_merge_launch()
        _check_launches(new_launch, old_launch)
        a = c["atm"]
        ref, rtg = oracle.cirsrad_ck_thermal(0, c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"], a["lay_press_pa"][0],
                                             a["lay_temp"][0], a["amount"][0], c["cont"][0], c["NLAYIN"], c["LAYINC"],
                                             c["SCALE"], c["EMTEMP"], -1.0, return_taugas=True)
        ref = np.squeeze(ref)
        print(f"cirsrad G={G} S={S} positive={positive}: taugas {_relmax(tg, rtg):.3e} / {_relmax(tg0, rtg):.3e}, "
              f"spectrum {_relmax(spec, ref):.3e} / {_relmax(spec0, ref):.3e} (new / old vs oracle)")
        assert np.array_equal(tg, tg0) and np.array_equal(spec, spec0)
        for got in (tg, tg0):
            np.testing.assert_allclose(got, rtg, rtol=RTOL, atol=0)
        for got in (spec, spec0):
            np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0)


def test_fewer_tiles_than_waves(eng, oracle):
    """W = 64, L = 1 is one tile: every wave of the block but one leaves at once, and its sentinel rows are never read."""
    for G in (20, 32):
        rng = np.random.default_rng(640 + G)
        delg = _delg(G)
        k = _mixed_k(rng, 64, G, 1, 3)
        amount = 10.0 ** rng.uniform(19, 22, (3, 1))
        new = eng.k_overlap(delg, k, amount)
        new_launch = eng.last_merge_launch()
        with _legacy():
            old = eng.k_overlap(delg, k, amount)
            old_launch = eng.last_merge_launch()
        _check_launches(new_launch, old_launch)
        ref = oracle.k_overlap(delg, k, amount)
        print(f"one tile G={G}: max rel err {_relmax(new, ref):.3e}, bits equal {np.array_equal(new, old)}")
        assert np.array_equal(new, old)
        np.testing.assert_allclose(new, ref, rtol=RTOL, atol=0)


def test_batch_of_models(eng, oracle):
    from archnemesis_dist_amd import synthetic as syn
    W, G, S, L, NP, NT, n = 70, 20, 3, 4, 4, 3, 3
    rng = np.random.default_rng(77)
    delg = _delg(G)
    PRESS, TEMP, _ = syn.synth_ktable(8, G, NP, NT, S, seed=21)
    K = np.ascontiguousarray(_mixed_k(rng, W, G, NP * NT, S, positive=True).reshape(W, G, NP, NT, S))
    WAVE = 300.0 + np.arange(W) * 1.0
    atm = syn.synth_atmosphere(L, S, seed=22)
    lp = np.repeat(atm["lay_press_pa"][:1], n, axis=0)
    lt = np.stack([atm["lay_temp"][0] + 3.0 * i for i in range(n)])
    am = np.stack([atm["amount"][0] * (1.0 + 0.25 * i) for i in range(n)])
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, 10.0)
    cont = np.repeat(syn.synth_continuum(W, L)[:1], n, axis=0)
    EMTEMP = lt[:, LAYINC[:, 0]][:, :, None]
    eng.upload_ktable(K, PRESS, TEMP, WAVE, delg)
    out = eng.cirsrad_ck_thermal(0, lp, lt, am, cont, NLAYIN, LAYINC, SCALE, EMTEMP, np.full(n, -1.0))
    new_launch = eng.last_merge_launch()
    with _legacy():
        out0 = eng.cirsrad_ck_thermal(0, lp, lt, am, cont, NLAYIN, LAYINC, SCALE, EMTEMP, np.full(n, -1.0))
        old_launch = eng.last_merge_launch()
    _check_launches(new_launch, old_launch)
    assert np.array_equal(out, out0)
    for i in range(n):
        ref = oracle.cirsrad_ck_thermal(0, K, PRESS, TEMP, WAVE, delg, lp[i], lt[i], am[i], cont[i], NLAYIN, LAYINC, SCALE,
                                        EMTEMP[i], -1.0)
        print(f"model {i}: max rel err {_relmax(out[i], ref):.3e}")
        np.testing.assert_allclose(out[i], ref, rtol=RTOL, atol=0)
