"""The forward merge kernel's whole walks on the launch's static schedule (merge_rowmajor_static): the library as it
launches by default against ANSFM_MERGE_STATIC=0 (the same kernel, the per-lane step of merge_rowmajor) bit for bit, against the
CPU oracle at the 1e-11 of tests/test_merge_rowmajor.py, and last_merge_static(), the (wave, merge) pairs walked on the schedule
and whether the launch carried a valid one, against what each table was built for.

A launch that carries the schedule walks every whole walk on it, so within one launch the count equals last_merge_rowmajor()'s
walked merges; where a count is asserted exactly the table is one tile of the default lane mapping (W = 1, L = 64: the 64 rows
of one wavenumber are one wave), and tests/test_merge_rowmajor_model.py decides every lane."""
import re
import os

import numpy as np
import pytest

from test_merge_rowmajor import RTOL, _delg, _env, _geometric_k, _model_passes, _same
from test_merge_rowmajor_model import list_len
from test_merge_static_model import interior_delg, invalid_delg, schedule_model
from test_merge_trim import _sweep_k  # noqa: E402  (random; flat to 1e-9; leading zeros; a zero gas in some cells)

pytestmark = pytest.mark.gpu

ONE_TILE = (1, 64)                                  # W, L


def _min_list():
    """kStaticMinList as the kernels are compiled with it"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "archnemesis_dist_amd", "csrc")
    return int(re.search(r"constexpr int kStaticMinList = (\d+);", open(os.path.join(csrc, "ansfm_merge_plan.h")).read()).group(1))


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


def _on_and_off(eng, run, carried=True):
    """run() by default and with ANSFM_MERGE_STATIC=0, compared bit for bit: the default result, its (static merges, valid) and
    its (walked, merged).  The switch changes neither the launch report nor `valid`; a launch that carries the schedule walks
    every whole walk on it, one that does not counts nothing.  (The merges walked whole may differ between the two launches:
    the second one hands a block's wavenumbers out in the order of the first one's pattern bytes.)"""
    with _env(ANSFM_MERGE_STATIC=""):
        new = run()
        launch, walked, static = eng.last_merge_launch(), eng.last_merge_rowmajor(), eng.last_merge_static()
    with _env(ANSFM_MERGE_STATIC="0"):
        off = run()
        off_launch, off_walked, off_static = eng.last_merge_launch(), eng.last_merge_rowmajor(), eng.last_merge_static()
    assert _same(new, off), "static on / off differ"
    assert launch == off_launch and walked[1] == off_walked[1], (launch, off_launch, walked, off_walked)
    assert off_static == (0, static[1]), (static, off_static)
    assert static == ((walked[0], True) if carried else (0, False)), (static, walked)
    return new, static, walked


def _run_overlap(eng, oracle, delg, k, amount, carried=True):
    tau, static, walked = _on_and_off(eng, lambda: eng.k_overlap(delg, k, amount), carried)
    np.testing.assert_allclose(tau, oracle.k_overlap(delg, k, amount), rtol=RTOL, atol=0)
    return static, walked


@pytest.mark.parametrize("G", [20, 17])
def test_counts_on_one_tile(eng, oracle, G):
    """Gas 1 six decades below gas 0, either way round and mixed over the lanes (swapped and unswapped lanes in one wave): the
    wave walks the merge on the schedule; with one lane of equal magnitudes it does not, and the list's results are the same."""
    W, L = ONE_TILE
    S = 2
    delg = _delg(G)
    rng = np.random.default_rng(61 + G)
    amount = 10.0 ** rng.uniform(20, 20.1, (S, L))
    apart = _geometric_k(rng, W, G, L, S, [0, -6])
    apart_sw = apart[..., ::-1].copy()
    mixed = np.where((np.arange(L) % 3 == 0)[None, None, :, None], apart_sw, apart)
    one_out = mixed.copy()
    one_out[0, :, 17, :] = _geometric_k(rng, W, G, L, S, [0, 0])[0, :, 17, :]
    for name, k, want in (("apart", apart, 1), ("apart, b the larger", apart_sw, 1), ("mixed orientations", mixed, 1),
                          ("one lane out", one_out, 0)):
        ok = _model_passes(oracle, delg, k, amount)[0]
        assert ok.all() if want else (ok.sum() == ok.size - 1 and not ok[0, 17]), name
        with _env(ANSFM_MERGE_LANES=""):
            static, walked = _run_overlap(eng, oracle, delg, k, amount)
        print(f"G={G} {name}: static / valid = {static}, walked / merged = {walked}")
        assert static == (want, True) and walked == (want, 1), (name, static, walked)


@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("shape", [(2, 1), (70, 3), (70, 33), (64, 100)], ids=lambda s: f"W{s[0]}L{s[1]}")
def test_shapes_through_the_seam(eng, oracle, shape, S):
    """The k_overlap seam over pad lanes, one row, rows that do not fill a tile and the benchmark's 100 rows, two and eight
    gases, in both lane mappings.  The first 64 wavenumbers (the first half where there are no more) have their gases far apart,
    the larger one alternately a and b; the others have similar magnitudes: walked and listed merges, swapped and unswapped
    lanes meet in one launch.  0 < static < merged wherever the mapping has a wave of each kind: a wave is 64 consecutive cells,
    wavenumber by wavenumber with the rows fastest (so from 64 far cells on) or, ANSFM_MERGE_LANES=wavenumbers, 64 wavenumbers
    of one row (so from W > 64); W = 2, L = 1 is one wave either way."""
    W, L = shape
    G = 20
    rng = np.random.default_rng(500 * W + L + S)
    delg = _delg(G)
    far = min(64, W // 2) if W <= 64 else 64
    k = _geometric_k(rng, W, G, L, S, [(-9 * s if s % 2 else 2 * s) for s in range(S)])
    k[far:] = _geometric_k(rng, W - far, G, L, S, rng.uniform(-0.5, 0.5, S))
    amount = 10.0 ** rng.uniform(20, 20.1, (S, L))
    for lanes in ("", "wavenumbers"):
        with _env(ANSFM_MERGE_LANES=lanes):
            static, walked = _run_overlap(eng, oracle, delg, k, amount)
        print(f"W={W} L={L} S={S} lanes={lanes or 'rows'}: static / valid = {static}, walked / merged = {walked}")
        if (W > 64) if lanes else (far * L >= 64):
            assert 0 < static[0] < walked[1], (static, walked)


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("G", [8, 12, 16, 17, 20, 32])
def test_list_lengths_and_weights(eng, oracle, G, f32):
    """G on both sides of a list length, and float64 weights, which have no table: nothing counted, no schedule.  The lists
    below kStaticMinList do not carry the form: they count 0 and still match.  Two tables: gases ten decades apart (every merge
    walks) and the four kinds of tests/test_merge_trim.py (ties from flat k(g), merged spectra not ascending, skip rules)."""
    W, L, S = 70, 3, 4
    rng = np.random.default_rng(13 * G + f32)
    delg = _delg(G, f32)
    carried = f32 and list_len(G) >= _min_list()
    amount = 10.0 ** rng.uniform(20, 20.1, (S, L))
    static, walked = _run_overlap(eng, oracle, delg, _geometric_k(rng, W, G, L, S, [0, -10, -20, 10]), amount, carried)
    if f32:
        assert walked[0] == walked[1] > 0, walked
    sweep, sweep_walked = _run_overlap(eng, oracle, delg, _sweep_k(rng, W, G, L, S), 10.0 ** rng.uniform(19, 22, (S, L)), carried)
    print(f"G={G} f32={f32}: static / valid = {static} of {walked}, sweep table {sweep} of {sweep_walked}")


@pytest.mark.parametrize("kind", ["interior", "invalid"])
def test_other_weights(eng, oracle, kind):
    """The two constructed del_g of the model test at G = 20: crossings at interior columns, four in one row -- walked on the
    schedule; and weights whose walk runs ahead of the bin boundaries -- no valid schedule, the per-lane walk, 0 counted."""
    W, L, S, G = 70, 3, 4, 20
    delg64 = interior_delg(G) if kind == "interior" else invalid_delg(G)
    assert schedule_model(delg64)["valid"] == (kind == "interior")
    delg = delg64.astype(np.float32)
    rng = np.random.default_rng(71)
    amount = 10.0 ** rng.uniform(20, 20.1, (S, L))
    k = _geometric_k(rng, W, G, L, S, [0, -10, -20, 10])
    static, walked = _run_overlap(eng, oracle, delg, k, amount, kind == "interior")
    print(f"{kind}: static / valid = {static}, walked / merged = {walked}")
    # (a spectrum merged with the interior weights has three bins of nearly one value: its later merges keep the list)
    assert walked[1] > 0 and (static[0] > 0) == (kind == "interior"), (static, walked)


def test_skip_rule_between_two_walks(eng, oracle):
    """A gas that is zero in every third row between two walked merges: those lanes keep their spectrum and neither vote nor
    merge, the others walk on the schedule; three merges, three counted."""
    W, L = ONE_TILE
    G, S = 20, 4
    rng = np.random.default_rng(67)
    delg = _delg(G)
    k = _geometric_k(rng, W, G, L, S, [0, -6, -12, -18])
    k[:, :, ::3, 2] = 0.0
    amount = 10.0 ** rng.uniform(20, 20.1, (S, L))
    with _env(ANSFM_MERGE_LANES=""):
        static, walked = _run_overlap(eng, oracle, delg, k, amount)
    assert static == (3, True) and walked == (3, 3), (static, walked)


@pytest.mark.parametrize("dedup", [True, False])
def test_fused_batch_from_the_table(eng, oracle, dedup):
    """The table path (not FROM_K): three models at L = 4 that differ from the first in one layer each, with and without layer
    de-duplication, on a table whose gases are six decades apart."""
    from archnemesis_dist_amd import synthetic as syn
    W, G, S, L, NP, NT, n = 70, 20, 3, 4, 4, 3, 3
    delg = _delg(G)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=31)
    K = K * 10.0 ** (-6.0 * np.arange(S))
    WAVE = 300.0 + np.arange(W) * 1.0
    atm = syn.synth_atmosphere(L, S, seed=32)
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
        spec, static, walked = _on_and_off(eng, run)
        computed, total = eng.last_layer_rows()
    finally:
        eng.set_layer_dedup(True)
    print(f"dedup={dedup}: rows computed {computed} of {total}, static / valid = {static}, walked / merged = {walked}")
    assert total == n * L and (computed < total if dedup else computed == total)
    assert static[0] > 0
    for i in range(n):
        ref = oracle.cirsrad_ck_thermal(0, K, PRESS, TEMP, WAVE, delg, lp[i], lt[i], am[i], cont[i], NLAYIN, LAYINC, SCALE,
                                        EMTEMP[i], -1.0)
        np.testing.assert_allclose(spec[i], ref, rtol=RTOL, atol=0)
