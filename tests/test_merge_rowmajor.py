"""The forward merge kernel's list-free walk of row-major merges (merge_rowmajor): the library as it launches by
default against ANSFM_MERGE_ROWMAJOR=0 (the same kernel, walk off) and ANSFM_MERGE_LEGACY=1 (no trim), bit for bit, and against
the CPU oracle at the suite's 1e-11; and last_merge_rowmajor(), the (wave, merge) pairs that took the walk and all that merged.

Where a count is asserted exactly the table is one tile of the default lane mapping -- W = 2, L = 32: 2 wavenumbers x 32 rows
are one wave, the other tiles of the 64-wavenumber block hold pad cells only, which never merge -- with two gases, so that
the model of tests/test_merge_rowmajor_model.py decides every lane from the very doubles the kernel forms (k * amount) and
the wave takes the walk iff all 64 pass.  With ANSFM_MERGE_LANES=wavenumbers the same table is 32 waves of two lanes."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from test_merge_rowmajor_model import lane_passes, tie_operands
from test_merge_trim import _sweep_k  # noqa: E402  (random; flat to 1e-9; leading zeros; a zero gas in some cells)

pytestmark = pytest.mark.gpu

RTOL = 1e-11
ROWMAJOR, LANE_ROWS = 64, 32                        # bits of ansfm_last_merge_launch's trims


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


@contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _delg(G, f32=True):
    """Gauss-Legendre weights; f32: as a float32 array, which is what makes the engine (and NumPy) form float32 products"""
    from archnemesis_dist_amd import synthetic as syn
    delg = syn.gauss_legendre_01(G, as_float32=f32)[1]
    return delg.astype(np.float32) if f32 else delg


def _same(a, b):
    if isinstance(a, tuple):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def _three_ways(eng, run, f32=True):
    """run() by default, with the walk off and without the trims: the default result and its (walked, merged) counts, after
    the three are compared bit for bit and the launch reports are checked"""
    with _env(ANSFM_MERGE_ROWMAJOR=""):             # not "0": the library's own choice
        new = run()
        launch, counts = eng.last_merge_launch(), eng.last_merge_rowmajor()
    with _env(ANSFM_MERGE_ROWMAJOR="0"):
        off = run()
        off_launch, off_counts = eng.last_merge_launch(), eng.last_merge_rowmajor()
    with _env(ANSFM_MERGE_LEGACY="1"):
        legacy = run()
        legacy_launch, legacy_counts = eng.last_merge_launch(), eng.last_merge_rowmajor()
    assert legacy_launch == (1, 0) and legacy_counts == (0, 0), (legacy_launch, legacy_counts)
    assert off_launch == (launch[0], launch[1] & ~ROWMAJOR), (launch, off_launch)
    if f32:
        assert launch[1] & ROWMAJOR and launch[1] & 1, launch
        assert off_counts == (0, counts[1]), (counts, off_counts)
        assert 0 <= counts[0] <= counts[1], counts
    else:                                           # float64 weights: no table, no walk, nothing counted
        assert not launch[1] & ROWMAJOR and not launch[1] & 1, launch
        assert counts == (0, 0) and off_counts == (0, 0), (counts, off_counts)
    assert _same(new, off), "walk on / off differ"
    assert _same(new, legacy), "default / legacy differ"
    return new, counts


def _geometric_k(rng, W, G, L, S, decades):
    """Smooth sorted k(g): a geometric progression of ratio 1.5 with 10 % jitter per gas and cell, gas s scaled by
    10^decades[s]: neighbouring ordinates are at least 20 % apart, a gas spans three and a half decades at G = 20"""
    g = np.arange(G, dtype=np.float64)[None, :, None, None]
    k = 1e-24 * 1.5 ** g * rng.uniform(0.95, 1.05, (W, G, L, S)) * 10.0 ** np.asarray(decades, np.float64)[None, None, None, :]
    assert np.all(np.diff(k, axis=1) > 0)
    return k


def _model_passes(oracle, delg, k, amount):
    """[S-1][W][L] booleans: the model's verdict for every lane and merge; the merged spectrum before gas s is the oracle's
    merge of the gases before it (exact for s = 1: gas 0's k * amount)"""
    W, G, L, S = k.shape
    out = np.zeros((S - 1, W, L), bool)
    for s in range(1, S):
        a = k[..., 0] * amount[0][None, None, :] if s == 1 else oracle.k_overlap(delg, k[..., :s], amount[:s])
        b = k[..., s] * amount[s][None, None, :]
        for w in range(W):
            for l in range(L):
                out[s - 1, w, l] = lane_passes(a[w, :, l], b[w, :, l])
    return out


def _run_overlap(eng, oracle, delg, k, amount, f32=True):
    tau, counts = _three_ways(eng, lambda: eng.k_overlap(delg, k, amount), f32)
    np.testing.assert_allclose(tau, oracle.k_overlap(delg, k, amount), rtol=RTOL, atol=0)
    return counts


ONE_TILE = (2, 32)                                  # W, L


@pytest.mark.parametrize("lanes", ["rows", "wavenumbers"])
def test_counts_on_one_tile(eng, oracle, lanes):
    """(a) gases eight decades apart, either way round and mixed over the lanes of the wave (swapped and unswapped lanes
    together): every wave walks; (b) gases of equal magnitude: none; (c) all lanes eight decades apart but one: that
    lane's wave does not walk and is not counted.  The model confirms what each table claims before the kernel is asked."""
    W, L = ONE_TILE
    G, S = 20, 2
    delg = _delg(G)
    rng = np.random.default_rng(41)
    amount = 10.0 ** rng.uniform(19, 22, (S, L))
    nwaves = 1 if lanes == "rows" else L            # waves that hold a real cell
    apart = _geometric_k(rng, W, G, L, S, [0, -12])                     # amounts differ by up to 3 decades: >= 8 remain
    apart_sw = apart[..., ::-1].copy()
    mixed = np.where((np.arange(L) % 3 == 0)[None, None, :, None], apart_sw, apart)
    equal = _geometric_k(rng, W, G, L, S, [0, 0])
    one_out = apart.copy()
    one_out[1, :, 17, :] = equal[1, :, 17, :]
    with _env(ANSFM_MERGE_LANES="" if lanes == "rows" else "wavenumbers"):
        for name, k, passing in (("apart", apart, "all"), ("apart, b the larger", apart_sw, "all"), ("mixed orientations", mixed, "all"),
                                 ("equal", equal, "none"), ("one lane out", one_out, "all but one")):
            ok = _model_passes(oracle, delg, k, amount)[0]
            assert {"all": ok.all(), "none": not ok.any(), "all but one": ok.sum() == ok.size - 1 and not ok[1, 17]}[passing], name
            walked = {"all": nwaves, "none": 0, "all but one": nwaves - 1}[passing]
            counts = _run_overlap(eng, oracle, delg, k, amount)
            print(f"{name} ({lanes}): walked / merged = {counts}")
            assert counts == (walked, nwaves), (name, counts)


@pytest.mark.parametrize("G", [8, 12, 16, 17, 20, 32])
def test_ties_flat_and_equal_rows(eng, oracle, G):
    """(d) the model test's tie constructions as tables of one tile, amount 1 so that the kernel's operands are the
    constructed doubles: r_i + c_{G-1} = r_{i+1} + c_0 in the top 53 bits (walked with b as the rows, not with a), flat
    operands, equal neighbouring rows -- the count is the model's verdict, the results are the list's bit for bit."""
    W, L = ONE_TILE
    delg = _delg(G)
    amount = np.ones((2, L))
    cases = []
    for nudge in (0, 3, -1):
        r, c = tie_operands(G, nudge)
        cases += [(f"tie {nudge:+d}, rows a", r, c), (f"tie {nudge:+d}, rows b", c, r)]
    cases += [("flat, rows a", np.full(G, 3.5), np.full(G, 3.0)), ("flat, rows b", np.full(G, 3.0), np.full(G, 3.5))]
    rows = 1024.0 * np.repeat(np.arange(1.0, G // 2 + 2), 2)[:G]
    small = np.arange(1, G + 1) * 2.0 ** -45
    cases += [("equal rows, rows a", rows, small), ("equal rows, rows b", small, rows)]
    for name, a, b in cases:
        k = np.empty((W, G, L, 2))
        k[..., 0] = a[None, :, None]
        k[..., 1] = b[None, :, None]
        ok = _model_passes(oracle, delg, k, amount)[0]
        assert ok.all() or not ok.any()
        with _env(ANSFM_MERGE_LANES=""):
            tau, counts = _three_ways(eng, lambda: eng.k_overlap(delg, k, amount))
        print(f"G={G} {name}: model {bool(ok.all())}, walked / merged = {counts}")
        assert counts == (int(ok.all()), 1), (name, counts)
        np.testing.assert_allclose(tau, oracle.k_overlap(delg, k, amount), rtol=RTOL, atol=0)


@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("shape", [(2, 1), (70, 3), (70, 33), (64, 100)], ids=lambda s: f"W{s[0]}L{s[1]}")
def test_shapes_through_the_seam(eng, oracle, shape, S):
    """(g) the k_overlap seam (FROM_K) over pad lanes, one row, rows that do not fill a tile and the benchmark's 100 rows, two
    and eight gases, in both lane mappings: in the first half of the wavenumbers the gases are far apart, the larger one
    alternately a and b, in the other half of similar magnitude, so that swapped and unswapped lanes and walked and listed
    merges meet in one launch."""
    W, L = shape
    G = 20
    rng = np.random.default_rng(100 * W + L + S)
    delg = _delg(G)
    k = _geometric_k(rng, W, G, L, S, [(-9 * s if s % 2 else 2 * s) for s in range(S)])
    k[W // 2:] = _geometric_k(rng, W - W // 2, G, L, S, rng.uniform(-3, 3, S))     # the other half: nearly equal magnitudes
    amount = 10.0 ** rng.uniform(19, 21, (S, L))
    for lanes in ("", "wavenumbers"):
        with _env(ANSFM_MERGE_LANES=lanes):
            counts = _run_overlap(eng, oracle, delg, k, amount)
        print(f"W={W} L={L} S={S} lanes={lanes or 'rows'}: walked / merged = {counts}")
        assert counts[1] > 0
        if W >= 64 and not lanes:                   # tiles of 2 wavenumbers x 32 rows inside the first half walk some merges
            assert 0 < counts[0] < counts[1], counts


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("G", [8, 12, 16, 17, 20, 32])
def test_list_lengths_and_weights(eng, oracle, G, f32):
    """(f) G on both sides of a list length and (h) float64 weights, which keep the list: nothing counted, bit 64 clear.  Two
    tables: gases ten decades apart (every wave walks every merge with float32 weights) and the four kinds of
    tests/test_merge_trim.py (ties from flat k(g), merged spectra not ascending -- lanes kept unswapped --, skip rules)."""
    W, L, S = 70, 3, 4
    rng = np.random.default_rng(7 * G + f32)
    delg = _delg(G, f32)
    amount = 10.0 ** rng.uniform(19, 21, (S, L))
    k = _geometric_k(rng, W, G, L, S, [0, -10, -20, 10])
    counts = _run_overlap(eng, oracle, delg, k, amount, f32)
    if f32:
        assert counts[0] == counts[1] > 0, counts
    counts = _run_overlap(eng, oracle, delg, _sweep_k(rng, W, G, L, S), 10.0 ** rng.uniform(19, 22, (S, L)), f32)
    print(f"G={G} f32={f32}: sweep table walked / merged = {counts}")


def test_skip_rule_between_two_walks(eng, oracle):
    """(i) a gas whose last ordinate is 0 between two row-major merges: the merged spectrum is kept, the wave walks the
    merge before and the merge after and counts two."""
    W, L = ONE_TILE
    G, S = 20, 4
    rng = np.random.default_rng(43)
    delg = _delg(G)
    k = _geometric_k(rng, W, G, L, S, [0, -12, 0, -24])
    k[..., 2] = 0.0
    amount = 10.0 ** rng.uniform(19, 21, (S, L))
    with _env(ANSFM_MERGE_LANES=""):
        counts = _run_overlap(eng, oracle, delg, k, amount)
    assert counts == (2, 2), counts


@pytest.mark.parametrize("dedup", [True, False])
def test_fused_batch_from_the_table(eng, oracle, dedup):
    """(g) the table path (not FROM_K): three models at L = 4 that differ from the first in one layer each, with and without
    layer de-duplication, on a table whose gases are ten decades apart."""
    from archnemesis_dist_amd import synthetic as syn
    W, G, S, L, NP, NT, n = 70, 20, 3, 4, 4, 3, 3
    delg = _delg(G)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=21)
    K = K * 10.0 ** (-10.0 * np.arange(S))
    WAVE = 300.0 + np.arange(W) * 1.0
    atm = syn.synth_atmosphere(L, S, seed=22)
    lp = np.repeat(atm["lay_press_pa"][:1], n, axis=0)
    lt = np.repeat(atm["lay_temp"][:1], n, axis=0)
    am = np.repeat(atm["amount"][:1], n, axis=0)
    for i in range(1, n):
        lt[i, i] += 3.0 * i
        am[i, :, i] *= 1.0 + 0.25 * i
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, 10.0)
    cont = np.repeat(syn.synth_continuum(W, L)[:1], n, axis=0)
    EMTEMP = lt[:, LAYINC[:, 0]][:, :, None]
    eng.upload_ktable(K, PRESS, TEMP, WAVE, delg)
    eng.set_layer_dedup(dedup)
    try:
        run = lambda: eng.cirsrad_ck_thermal(0, lp, lt, am, cont, NLAYIN, LAYINC, SCALE, EMTEMP, np.full(n, -1.0))
        spec, counts = _three_ways(eng, run)
        computed, total = eng.last_layer_rows()
    finally:
        eng.set_layer_dedup(True)
    print(f"dedup={dedup}: rows computed {computed} of {total}, walked / merged = {counts}")
    assert total == n * L and (computed < total if dedup else computed == total)
    assert counts[1] > 0
    for i in range(n):
        ref = oracle.cirsrad_ck_thermal(0, K, PRESS, TEMP, WAVE, delg, lp[i], lt[i], am[i], cont[i], NLAYIN, LAYINC, SCALE,
                                        EMTEMP[i], -1.0)
        np.testing.assert_allclose(spec[i], ref, rtol=RTOL, atol=0)
