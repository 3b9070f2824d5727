"""The forward merge kernel's walk of the separable top rows of a list merge (merge_suffix_row): the library as it
launches by default against ANSFM_MERGE_SUFFIX=0 (the same kernel, the list to its end) bit for bit, against the CPU oracle at
the 1e-11 of tests/test_merge_rowmajor.py, and last_merge_suffix(), the rows walked behind a list phase, against the model of
tests/test_merge_suffix_model.py.

Where a count is asserted exactly the table is one tile of the default lane mapping -- W = 1, L = 64: the 64 rows of one
wavenumber are one wave, the other tiles of the block hold pad cells only, which never merge -- so that the model decides every
lane from the very doubles the kernel forms (k * amount; the merged spectrum before a later gas is the oracle's) and the wave
takes the largest i0 of its merging lanes.  The rule never gives i0 = 1 (boundaries 0 .. G-2 all passing is the whole walk), so
the smallest start row a wave can be built for is 2."""
import os
import re

import numpy as np
import pytest

from test_merge_rowmajor import RTOL, _delg, _env, _geometric_k, _same
from test_merge_rowmajor_model import lane_keys, list_len, swap_choice
from test_merge_suffix_model import MIN_LIST, gap_rows, lane_i0, start_row
from test_merge_trim import _sweep_k  # noqa: E402  (random; flat to 1e-9; leading zeros; a zero gas in some cells)

pytestmark = pytest.mark.gpu

ONE_TILE = (1, 64)                                  # W, L


def _min_rows():
    """kSuffixMinRows as the kernel is compiled with it (and kSuffixMinList is the model's)"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "archnemesis_dist_amd", "csrc")
    plan = open(os.path.join(csrc, "ansfm_merge_plan.h")).read()
    assert int(re.search(r"constexpr int kSuffixMinList = (\d+);", plan).group(1)) == MIN_LIST
    text = open(os.path.join(csrc, "ansfm_merge64.hip.h")).read()
    return int(re.search(r"constexpr int kSuffixMinRows = (\d+);", text).group(1))


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


def _on_and_off(eng, run, f32=True):
    """run() by default and with ANSFM_MERGE_SUFFIX=0, compared bit for bit: the default result and its (rows, rows of list
    merges).  The switch does not change the launch report.  (The merges walked whole may differ between the two launches:
    the second one hands a block's wavenumbers out in the order of the first one's pattern bytes, which regroups the tiles
    that straddle wavenumbers.)"""
    with _env(ANSFM_MERGE_SUFFIX=""):
        new = run()
        launch, walked, rows = eng.last_merge_launch(), eng.last_merge_rowmajor(), eng.last_merge_suffix()
    with _env(ANSFM_MERGE_SUFFIX="0"):
        off = run()
        off_launch, off_walked, off_rows = eng.last_merge_launch(), eng.last_merge_rowmajor(), eng.last_merge_suffix()
    assert _same(new, off), "suffix on / off differ"
    assert launch == off_launch and walked[1] == off_walked[1], (launch, off_launch, walked, off_walked)
    assert off_rows[0] == 0 and off_rows[1] % (rows[1] // (walked[1] - walked[0]) if rows[1] else 1) == 0, (rows, off_rows)
    if f32:
        assert launch[1] & 1 and launch[1] & 64, launch
        assert 0 <= rows[0] <= rows[1], rows
    else:                                           # float64 weights: no table, no walk, nothing counted
        assert not launch[1] & 1 and rows == (0, 0), (launch, rows)
    return new, rows, walked


def _model_rows(oracle, delg, k, amount):
    """(rows walked behind a list phase, rows of the merges not walked whole) of one tile, W = 1 and L <= 64: the skip rules,
    the orientation and i0 of every merging lane, the wave's start row"""
    W, G, L, S = k.shape
    assert W == 1 and L <= 64
    rows = listed = 0
    for s in range(1, S):
        a = k[0, :, :, 0] * amount[0][None, :] if s == 1 else oracle.k_overlap(delg, k[..., :s], amount[:s])[0]
        b = k[0, :, :, s] * amount[s][None, :]
        alast, blast = a[-1], b[-1]
        if s == 1:
            take_b = alast <= 0.0
            keep_a = ~take_b & (blast <= 0.0)
        else:
            keep_a = blast <= 0.0
            take_b = ~keep_a & (alast <= 0.0)
        merging = np.nonzero(~(take_b | keep_a))[0]
        if merging.size == 0:
            continue
        i0 = 0
        for l in merging:
            sw = swap_choice(a[:, l], b[:, l])
            r, c = (b[:, l], a[:, l]) if sw else (a[:, l], b[:, l])
            i0 = max(i0, lane_i0(lane_keys(r, c, sw)))
        start = start_row(i0, G, _min_rows())
        listed += G if start != 0 else 0
        rows += G - start if 0 < start < G else 0
    return rows, listed


def _run_overlap(eng, oracle, delg, k, amount, f32=True):
    tau, rows, walked = _on_and_off(eng, lambda: eng.k_overlap(delg, k, amount), f32)
    np.testing.assert_allclose(tau, oracle.k_overlap(delg, k, amount), rtol=RTOL, atol=0)
    return rows, walked


def _spread_k(rng, W, G, L, S, lo=-3.5, hi=-1.0):
    """_geometric_k with every gas after the first between `lo` and `hi` decades below it, drawn per wavenumber: the top rows
    of the larger operand stand clear of the smaller one from a row that differs from wavenumber to wavenumber"""
    k = _geometric_k(rng, W, G, L, S, np.zeros(S))
    dec = rng.uniform(lo, hi, (W, 1, 1, S))
    dec[..., 0] = 0.0
    return k * 10.0 ** dec


@pytest.mark.parametrize("G", [20, 17])
def test_start_rows_on_one_tile(eng, oracle, G):
    """Constructed operands, amount 1: every lane's i0 is 2, G/2 (rounded up: 9 at G = 17, an odd G * i0) or G-1, in both
    orientations and mixed over the lanes; one lane of the 64 alone at G/2 among lanes at 2 pulls the wave up.  The count is
    the model's."""
    W, L = ONE_TILE
    delg = _delg(G)
    amount = np.ones((2, L))
    c = np.linspace(0.0, 8.0, G)

    def table(i0_of_lane, rows_b_of_lane):
        k = np.empty((W, G, L, 2))
        for l in range(L):
            r = gap_rows(G, i0_of_lane[l])
            k[0, :, l, 0], k[0, :, l, 1] = (c, r) if rows_b_of_lane[l] else (r, c)
        return k

    lanes = np.arange(L)
    half = (G + 1) // 2
    one_up = np.full(L, 2)
    one_up[17] = half
    for name, i0s, sw in (("2", np.full(L, 2), lanes < 0), ("G/2", np.full(L, half), lanes < 0),
                          ("G-1", np.full(L, G - 1), lanes < 0), ("2, rows b", np.full(L, 2), lanes >= 0),
                          ("G/2, mixed orientations", np.full(L, half), lanes % 3 == 0),
                          ("2 and one lane at G/2", one_up, lanes % 2 == 0),
                          ("0, 2, G/2 by lane", np.array([0, 2, half])[lanes % 3], lanes % 2 == 0)):
        k = table(i0s, sw)
        want = _model_rows(oracle, delg, k, amount)
        start = start_row(int(i0s.max()), G, _min_rows())
        assert want == (G - start if start < G else 0, G), (name, want)
        with _env(ANSFM_MERGE_LANES=""):
            rows, walked = _run_overlap(eng, oracle, delg, k, amount)
        print(f"G={G} i0 {name}: rows walked behind the list / rows of list merges = {rows}")
        assert rows == want and walked == (0, 1), (name, rows, want, walked)


@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("shape", [(2, 1), (70, 3), (70, 33), (64, 100)], ids=lambda s: f"W{s[0]}L{s[1]}")
def test_shapes_through_the_seam(eng, oracle, shape, S):
    """Pad wavenumbers, one row, tiles that straddle two wavenumbers with different i0 and a tile tail, two and eight gases,
    in both lane mappings"""
    W, L = shape
    G = 20
    rng = np.random.default_rng(300 * W + L + S)
    delg = _delg(G)
    k = _spread_k(rng, W, G, L, S)
    amount = 10.0 ** rng.uniform(20, 20.1, (S, L))
    for lanes in ("", "wavenumbers"):
        with _env(ANSFM_MERGE_LANES=lanes):
            rows, walked = _run_overlap(eng, oracle, delg, k, amount)
        print(f"W={W} L={L} S={S} lanes={lanes or 'rows'}: suffix rows / list rows = {rows}, walked / merged = {walked}")
        assert 0 < rows[0] < rows[1], rows


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("G", [8, 12, 16, 17, 20, 32])
def test_list_lengths_and_weights(eng, oracle, G, f32):
    """G on both sides of a list length (8: a list without the partial form), odd G * i0, and float64 weights, which have no
    table: nothing counted, same results.
    Two tables: gases up to four decades apart and the four kinds of tests/test_merge_trim.py (ties from flat k(g), merged
    spectra not ascending, skip rules)."""
    W, L, S = 70, 3, 4
    rng = np.random.default_rng(11 * G + f32)
    delg = _delg(G, f32)
    amount = 10.0 ** rng.uniform(20, 20.1, (S, L))
    rows, _ = _run_overlap(eng, oracle, delg, _spread_k(rng, W, G, L, S), amount, f32)
    if f32 and list_len(G) >= MIN_LIST:
        assert 0 < rows[0] < rows[1], rows
    elif f32:                                       # the kernels of the short lists do not carry the partial form
        assert rows[0] == 0 < rows[1], rows
    sweep, _ = _run_overlap(eng, oracle, delg, _sweep_k(rng, W, G, L, S), 10.0 ** rng.uniform(19, 22, (S, L)), f32)
    print(f"G={G} f32={f32}: suffix rows / list rows = {rows}, sweep table {sweep}")


def test_skip_rule_between_two_partial_merges(eng, oracle):
    """A gas that is zero in some cells between two partial merges: those lanes keep their spectrum and do not vote, the
    others merge; the counts are the model's for all three merges."""
    W, L = ONE_TILE
    G, S = 20, 4
    rng = np.random.default_rng(47)
    delg = _delg(G)
    k = _spread_k(rng, W, G, L, S, -3.0, -1.0)
    k[:, :, ::3, 2] = 0.0
    amount = 10.0 ** rng.uniform(20, 20.1, (S, L))
    want = _model_rows(oracle, delg, k, amount)
    with _env(ANSFM_MERGE_LANES=""):
        rows, walked = _run_overlap(eng, oracle, delg, k, amount)
    print(f"suffix rows / list rows = {rows}, model {want}, walked / merged = {walked}")
    assert rows == want and walked[1] == 3 and rows[0] > 0, (rows, want, walked)


@pytest.mark.parametrize("dedup", [True, False])
def test_fused_batch_from_the_table(eng, oracle, dedup):
    """The table path (not FROM_K): three models at L = 4 that differ from the first in one layer each, with and without
    layer de-duplication, on a table whose gases are two decades apart."""
    from archnemesis_dist_amd import synthetic as syn
    W, G, S, L, NP, NT, n = 70, 20, 3, 4, 4, 3, 3
    delg = _delg(G)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=21)
    K = K * 10.0 ** (-2.0 * np.arange(S))
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
        spec, rows, walked = _on_and_off(eng, run)
        computed, total = eng.last_layer_rows()
    finally:
        eng.set_layer_dedup(True)
    print(f"dedup={dedup}: rows computed {computed} of {total}, suffix rows / list rows = {rows}, walked / merged = {walked}")
    assert total == n * L and (computed < total if dedup else computed == total)
    assert rows[1] > 0
    for i in range(n):
        ref = oracle.cirsrad_ck_thermal(0, K, PRESS, TEMP, WAVE, delg, lp[i], lt[i], am[i], cont[i], NLAYIN, LAYINC, SCALE,
                                        EMTEMP[i], -1.0)
        np.testing.assert_allclose(spec[i], ref, rtol=RTOL, atol=0)


def test_off_with_the_walk(eng, oracle):
    """ANSFM_MERGE_ROWMAJOR=0 switches the partial form off with the walk: no row is counted, the results are the same bits."""
    W, L = ONE_TILE
    G = 20
    rng = np.random.default_rng(53)
    delg = _delg(G)
    k = _spread_k(rng, W, G, L, 2, -3.0, -1.0)
    amount = 10.0 ** rng.uniform(20, 20.1, (2, L))
    with _env(ANSFM_MERGE_LANES="", ANSFM_MERGE_ROWMAJOR=""):
        tau = eng.k_overlap(delg, k, amount)
        rows = eng.last_merge_suffix()
    with _env(ANSFM_MERGE_LANES="", ANSFM_MERGE_ROWMAJOR="0"):
        off = eng.k_overlap(delg, k, amount)
        off_launch, off_rows = eng.last_merge_launch(), eng.last_merge_suffix()
    assert rows == _model_rows(oracle, delg, k, amount) and rows[0] > 0, rows
    assert not off_launch[1] & 64 and off_rows == (0, G), (off_launch, off_rows)
    assert np.array_equal(tau, off)
