"""The forward merge kernel with a wave cut along one wavenumber, 64 rows deep (the group width of the row
mapping is run-time data of k_ck_overlap): the library's own choice (width 1), ANSFM_MERGE_LANES=pairs (2 wavenumbers x 32
rows), ANSFM_MERGE_LANES=wavenumbers (64 wavenumbers of one row) and ANSFM_MERGE_LEGACY=1 (no trim), all four bit for bit, and
against the CPU oracle at the suite's 1e-11.  ansfm_last_merge_group_width must report 1 / 2 / 0 / 0, and the trims word of
ansfm_last_merge_launch carries no bit for the width: bit 32 is set for both row mappings.

The tables are built from the two halves of tests/test_merge_rowmajor.py's _geometric_k: in the first half of the wavenumbers
the gases lie far apart, the larger one alternately a and b (a tile inside it walks), in the other half they are of equal
magnitude (no lane passes the test there), so that walked and listed merges and both orientations meet in one launch."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from test_merge_rowmajor import _geometric_k  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-11
LANE_ROWS, ROWMAJOR = 32, 64                       # bits of ansfm_last_merge_launch's trims
WAYS = (("", 1), ("pairs", 2), ("wavenumbers", 0))  # ANSFM_MERGE_LANES and the width the launch must report


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
    from archnemesis_dist_amd import synthetic as syn
    delg = syn.gauss_legendre_01(G, as_float32=f32)[1]
    return delg.astype(np.float32) if f32 else delg


def _same(a, b):
    if isinstance(a, tuple):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def _four_ways(eng, run, f32=True):
    """run() as the library launches it by its own choice, with pairs, over wavenumbers and without the trims: the first
    result and its (walked, merged) counts, after the four are compared bit for bit and the launch reports are checked"""
    results, launches, counts = [], [], []
    for lanes, width in WAYS:
        with _env(ANSFM_MERGE_LANES=lanes):
            results.append(run())
            launches.append(eng.last_merge_launch())
            counts.append(eng.last_merge_rowmajor())
            assert eng.last_merge_group_width() == width, (lanes, eng.last_merge_group_width())
    with _env(ANSFM_MERGE_LANES="", ANSFM_MERGE_LEGACY="1"):
        legacy = run()
        assert eng.last_merge_launch() == (1, 0)
        assert eng.last_merge_group_width() == 0
    one, pairs, waves = launches
    assert one[1] & LANE_ROWS and one[1] & 8 and one[1] & 16, one
    assert pairs == one, (one, pairs)              # the width is no bit of the trims
    assert waves == (one[0], one[1] & ~LANE_ROWS), (one, waves)
    if f32:
        assert one[1] & ROWMAJOR and one[1] & 1, one
        assert all(0 <= c[0] <= c[1] for c in counts), counts
    else:                                           # float64 weights: no table, the same mapping, nothing counted
        assert not one[1] & ROWMAJOR and not one[1] & 1, one
        assert all(c == (0, 0) for c in counts), counts
    for name, other in (("pairs", results[1]), ("wavenumbers", results[2]), ("legacy", legacy)):
        assert _same(results[0], other), f"width 1 / {name} differ"
    return results[0], counts[0]


def _seam_table(W, G, L, S):
    rng = np.random.default_rng(100 * W + L + S + 7 * G)
    k = _geometric_k(rng, W, G, L, S, [(-9 * s if s % 2 else 2 * s) for s in range(S)])
    if W >= 2:
        k[W // 2:] = _geometric_k(rng, W - W // 2, G, L, S, np.zeros(S))     # the other half: equal magnitudes, no walk
    amount = 10.0 ** rng.uniform(19, 21, (S, L))
    return k, amount


def _run_seam(eng, oracle, W, L, S, G, f32=True):
    delg = _delg(G, f32)
    k, amount = _seam_table(W, G, L, S)
    tau, counts = _four_ways(eng, lambda: eng.k_overlap(delg, k, amount), f32)
    ref = oracle.k_overlap(delg, k, amount)
    err = float(np.max(np.abs(tau - ref) / np.maximum(np.abs(ref), 1e-300)))
    print(f"W={W} L={L} S={S} G={G} f32={f32}: vs oracle {err:.3e}, walked / merged = {counts}")
    np.testing.assert_allclose(tau, ref, rtol=RTOL, atol=0)
    return counts


@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("shape", [(1, 1), (2, 32), (3, 64), (70, 3), (70, 33), (70, 65), (64, 100)], ids=lambda s: f"W{s[0]}L{s[1]}")
def test_shapes_through_the_seam(eng, oracle, shape, S):
    """The k_overlap seam (FROM_K) at G = 20: one cell; the one tile both widths share; one tile per wavenumber exactly; rows
    that do not fill a tile, so that a tile spans 21 wavenumbers; 33 and 65 rows, where every tile runs on into the next
    wavenumber; and the benchmark's 100 rows."""
    W, L = shape
    counts = _run_seam(eng, oracle, W, L, S, 20)
    assert counts[1] > 0
    if W >= 64:                                     # tiles inside the far-apart half walk, tiles inside the other do not
        assert 0 < counts[0] < counts[1], counts


@pytest.mark.parametrize("G", [8, 12, 20, 32])
def test_list_lengths(eng, oracle, G):
    """G on both sides of a list length at (W, L) = (70, 3), four gases"""
    counts = _run_seam(eng, oracle, 70, 3, 4, G)
    assert 0 < counts[0] < counts[1], counts


@pytest.mark.parametrize("shape", [(70, 3), (70, 65)], ids=lambda s: f"W{s[0]}L{s[1]}")
def test_float64_weights(eng, oracle, shape):
    """float64 weights keep the kernel without the weight table and the walk: the same mapping, the same results"""
    W, L = shape
    assert _run_seam(eng, oracle, W, L, 4, 20, f32=False) == (0, 0)


@pytest.mark.parametrize("dedup", [True, False])
def test_fused_batch_from_the_table(eng, oracle, dedup):
    """The table path (not FROM_K): three models at L = 4 that differ from the first in one layer each, with and without
    layer de-duplication (8 or 12 rows: a tile spans eight or five wavenumbers)."""
    from archnemesis_dist_amd import synthetic as syn
    W, G, S, L, NP, NT, n = 70, 20, 3, 4, 4, 3, 3
    delg = _delg(G)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=21)
    K[:W // 2] *= 10.0 ** (-10.0 * np.arange(S))   # gases ten decades apart; the other half: the generator's own magnitudes
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
        spec, counts = _four_ways(eng, run)
        computed, total = eng.last_layer_rows()
    finally:
        eng.set_layer_dedup(True)
    print(f"dedup={dedup}: rows computed {computed} of {total}, walked / merged = {counts}")
    assert total == n * L and (computed < total if dedup else computed == total)
    # W = 70: tiles inside the first half, ten decades apart, walk; tiles of the generator's own magnitudes keep the list
    assert 0 < counts[0] < counts[1], counts
    for i in range(n):
        ref = oracle.cirsrad_ck_thermal(0, K, PRESS, TEMP, WAVE, delg, lp[i], lt[i], am[i], cont[i], NLAYIN, LAYINC, SCALE,
                                        EMTEMP[i], -1.0)
        np.testing.assert_allclose(spec[i], ref, rtol=RTOL, atol=0)
