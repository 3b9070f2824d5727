"""The fast path of the forward merge kernel with its three later trims (the pair weight from a product table
shared by a block of several waves per CU, the two-instruction key repack, and whichever else of the constants is on) against the
code without them (ANSFM_MERGE_LEGACY=1: one-wave blocks, the weight from its two factors, the old packing) bit for bit, and
both against the CPU oracle at the suite's 1e-11:
  * every instantiated list length, with and without padding entries, float32 and float64 weights, the four input kinds of
    tests/test_merge_trim.py, through the array-level k_overlap and through the fused CIRSrad forward model;
  * the block of several waves: fewer tiles than waves, more tiles than one block's waves, a batch of models;
  * merged elements that close a bin in consecutive steps."""
import os
from contextlib import contextmanager

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


def _block_waves(G, cap=8):
    """Waves of the one block per CU: what fits 160 KiB beside DG / GORD / the float32 copy and the (G + 1) x 32 table."""
    shared = (2 * 32 + 2) * 8 + 32 * 4 + (G + 1) * 32 * 8
    return min(cap, (160 * 1024 - shared) // ((2 * G + 1) * 64 * 8))


def _check_launches(new_launch, old_launch, G, f32):
    """The comparison is between two kernels only if the first run took the trimmed fast path: some trim bit set, with float32
    weights the table (bit 1) in a block of several waves, with float64 weights one-wave blocks; and the second run none."""
    waves, trims = new_launch
    assert trims != 0, new_launch
    if f32:
        assert trims & 1 and waves == _block_waves(G) and waves > 1, new_launch
    else:
        assert not trims & 1 and waves == 1, new_launch
    assert old_launch == (1, 0), old_launch


def _delg(G, f32):
    """Gauss-Legendre weights; f32: as a float32 ARRAY, which is what makes the engine (and NumPy) form float32 products --
    synthetic.gauss_legendre_01 only rounds the values and hands them back as float64."""
    from archnemesis_dist_amd import synthetic as syn
    _, delg = syn.gauss_legendre_01(G, as_float32=f32)
    return delg.astype(np.float32) if f32 else delg


def _relmax(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def _sweep_k(rng, W, G, L, S):
    """The four input kinds of tests/test_merge_trim.py::_sweep_k along the wavenumber axis: random; flat to 1e-9 (the
    reorder of merge_init); the low g-ordinates of one gas zero in some columns; one gas zero altogether in some cells
    (the skip rules)."""
    k = np.sort(10.0 ** rng.uniform(-25, -20, (W, G, L, S)), axis=1)
    q = W // 4
    g = np.arange(G, dtype=np.float64)[None, :, None, None]
    k[q:2 * q] = 10.0 ** rng.uniform(-24, -21, (q, 1, L, S)) * (1.0 + g * 1e-9 / G)
    ncut = rng.integers(1, max(2, G // 2), size=(q, 1, L))
    s0 = S // 2
    k[2 * q:3 * q, :, :, s0] = np.where(np.arange(G)[None, :, None] < ncut, 0.0, k[2 * q:3 * q, :, :, s0])
    k[3 * q:, :, 0, 0] = 0.0
    k[3 * q:, :, L - 1, S - 1] = 0.0
    return k


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("G", G_SWEEP)
def test_k_overlap_old_and_new_paths(eng, oracle, G, S, f32):
    rng = np.random.default_rng(8100 + 10 * G + S)
    W, L = 136, 3                                  # two full tiles and one with pad lanes
    delg = _delg(G, f32)
    k = _sweep_k(rng, W, G, L, S)
    amount = 10.0 ** rng.uniform(19, 22, (S, L))
    new = eng.k_overlap(delg, k, amount)
    new_launch = eng.last_merge_launch()
    with _legacy():
        old = eng.k_overlap(delg, k, amount)
        old_launch = eng.last_merge_launch()
    _check_launches(new_launch, old_launch, G, f32)
    ref = oracle.k_overlap(delg, k, amount)
    print(f"k_overlap G={G} S={S} f32={f32}: new vs oracle {_relmax(new, ref):.3e}, old vs oracle {_relmax(old, ref):.3e}, "
          f"bits equal {np.array_equal(new, old)}")
    assert np.array_equal(new, old)
    np.testing.assert_allclose(new, ref, rtol=RTOL, atol=0)
    np.testing.assert_allclose(old, ref, rtol=RTOL, atol=0)


def _cirsrad_case(rng, W, G, S, L, f32, positive):
    """A forward model whose k-table columns are the four kinds of _sweep_k (positive: the first two only, i.e. a table
    without a boxed entry, which is read without the box tests)."""
    from archnemesis_dist_amd import synthetic as syn
    NP, NT = 3, 2
    delg = _delg(G, f32)
    PRESS, TEMP, _ = syn.synth_ktable(8, G, NP, NT, S, seed=5)
    kk = _sweep_k(rng, W, G, NP * NT, S)
    if positive:
        h = W // 2
        kk[h:] = kk[:W - h]
    K = np.ascontiguousarray(kk.reshape(W, G, NP, NT, S))
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


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("G", G_SWEEP)
def test_cirsrad_old_and_new_paths(eng, oracle, G, S, f32):
    rng = np.random.default_rng(9100 + 10 * G + S)
    for positive in (True, False):
        c = _cirsrad_case(rng, 136, G, S, 3, f32, positive)
        eng.upload_ktable(c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"])
        assert eng.ktable_info()[1]                # monotone: the fast path
        assert eng.ktable_has_boxed() is (not positive)
        spec, tg = _run_cirsrad(eng, c)
        new_launch = eng.last_merge_launch()
        with _legacy():
            spec0, tg0 = _run_cirsrad(eng, c)
            old_launch = eng.last_merge_launch()
        _check_launches(new_launch, old_launch, G, f32)
        a = c["atm"]
        ref, rtg = oracle.cirsrad_ck_thermal(0, c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"], a["lay_press_pa"][0],
                                             a["lay_temp"][0], a["amount"][0], c["cont"][0], c["NLAYIN"], c["LAYINC"],
                                             c["SCALE"], c["EMTEMP"], -1.0, return_taugas=True)
        ref = np.squeeze(ref)
        print(f"cirsrad G={G} S={S} f32={f32} positive={positive}: taugas {_relmax(tg, rtg):.3e} / {_relmax(tg0, rtg):.3e}, "
              f"spectrum {_relmax(spec, ref):.3e} / {_relmax(spec0, ref):.3e} (new / old vs oracle)")
        assert np.array_equal(tg, tg0) and np.array_equal(spec, spec0)
        for got in (tg, tg0):
            np.testing.assert_allclose(got, rtg, rtol=RTOL, atol=0)
        for got in (spec, spec0):
            np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0)


@pytest.mark.parametrize("W", [64, 64 * 9])
def test_block_of_waves_fewer_and_more_tiles_than_waves(eng, oracle, W):
    """W = 64, L = 1 is one tile: every wave of the one block but one finds the queues empty and leaves at once.  W = 576 is
    nine tiles: more than the waves of one block at any list length."""
    for G in (20, 32):
        rng = np.random.default_rng(500 + W + G)
        delg = _delg(G, True)
        k = np.sort(10.0 ** rng.uniform(-25, -20, (W, G, 1, 3)), axis=1)
        amount = 10.0 ** rng.uniform(19, 22, (3, 1))
        tau = eng.k_overlap(delg, k, amount)
        waves, trims = eng.last_merge_launch()
        assert waves == _block_waves(G) and trims & 1, (waves, trims)
        ref = oracle.k_overlap(delg, k, amount)
        print(f"W={W} G={G}: max rel err {_relmax(tau, ref):.3e}")
        np.testing.assert_allclose(tau, ref, rtol=RTOL, atol=0)


def test_block_of_waves_batch_of_models(eng, oracle):
    from archnemesis_dist_amd import synthetic as syn
    W, G, S, L, NP, NT, n = 70, 20, 3, 4, 4, 3, 3
    delg = _delg(G, True)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=21)
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
    waves, trims = eng.last_merge_launch()
    assert waves == _block_waves(G) and trims & 1, (waves, trims)
    for i in range(n):
        ref = oracle.cirsrad_ck_thermal(0, K, PRESS, TEMP, WAVE, delg, lp[i], lt[i], am[i], cont[i], NLAYIN, LAYINC, SCALE,
                                        EMTEMP[i], -1.0)
        print(f"model {i}: max rel err {_relmax(out[i], ref):.3e}")
        np.testing.assert_allclose(out[i], ref, rtol=RTOL, atol=0)


def _consecutive_crossings(delg, a, b):
    """rank()'s walk over the sorted sums of one cell, restated: how often two consecutive elements each close a bin."""
    G = len(delg)
    dg = np.asarray(delg)
    w = (dg[:, None] * dg[None, :]).astype(np.float64).ravel()       # float32 product when del_g is float32
    order = np.argsort((a[:, None] + b[None, :]).ravel(), kind="stable")
    g_ord = np.concatenate([[0.0], np.cumsum(dg).astype(np.float64)])
    g_ord[G] = 1.0
    ig, gd, prev, pairs = 0, 0.0, False, 0
    for t in order:
        gd += w[t]
        cross = ig < G and gd >= g_ord[ig + 1]
        if cross:
            ig += 1
            pairs += prev
        prev = cross
    return pairs


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("G", [8, 20])
def test_bins_closed_in_consecutive_steps(eng, oracle, G, f32):
    """One gas 1e6 times the other, so the merged order runs through the columns one by one; two bins of width 1e-4 among
    wide ones and weights that sum to 0.9, so the walk falls behind the column ends and an element of a wide column steps
    over three boundaries at once: the two elements after it close a bin each."""
    rng = np.random.default_rng(40 + G)
    delg = np.full(G, 0.9 / (G - 2))
    delg[2] = delg[3] = 1e-4
    if f32:
        delg = delg.astype(np.float32)
    W, L, S = 70, 2, 2
    k = np.empty((W, G, L, S))
    k[..., 0] = np.sort(10.0 ** rng.uniform(-25, -20, (W, G, L)), axis=1)
    k[..., 1] = np.sort(10.0 ** rng.uniform(-14, -12, (W, G, L)), axis=1)
    assert k[..., 1].min() >= 1e6 * k[..., 0].max()
    amount = np.full((S, L), 1e20)
    # the oracle returns the binned spectrum only, so the walk is restated here (and its result below is the oracle's): every cell
    pairs = min(_consecutive_crossings(delg, k[w, :, l, 0] * 1e20, k[w, :, l, 1] * 1e20) for w in range(W) for l in range(L))
    print(f"G={G} f32={f32}: at least {pairs} pairs of consecutive elements that each close a bin in every cell")
    assert pairs >= 1
    new = eng.k_overlap(delg, k, amount)
    new_launch = eng.last_merge_launch()
    with _legacy():
        old = eng.k_overlap(delg, k, amount)
        old_launch = eng.last_merge_launch()
    _check_launches(new_launch, old_launch, G, f32)
    ref = oracle.k_overlap(delg, k, amount)
    print(f"max rel err {_relmax(new, ref):.3e}")
    assert np.array_equal(new, old)
    np.testing.assert_allclose(new, ref, rtol=RTOL, atol=0)
