"""The wavenumber order of the forward merge (ansfm_last_merge_order): a launch of the library's own choice
writes one pattern byte per wavenumber, the row-major verdicts of its merges at the middle row, and hands the wavenumbers of a
64-block out sorted by the bytes of the launch before while that launch had the same source, W, rows, S and G.

The table decides the verdict by construction: in even wavenumbers gas s lies ten decades below gas s - 1, so every lane
passes merge_rowmajor_test in every merge; in odd wavenumbers the gases are of equal magnitude, so none passes.  The model of
tests/test_merge_rowmajor_model.py confirms that before the kernel is asked.  W = 70: one full block and one of six real and
58 pad wavenumbers.  The order changes which wave holds a cell and nothing in what is computed for it: every result is
compared bit for bit with ANSFM_MERGE_ORDER=0, ANSFM_MERGE_ROWMAJOR=0 and ANSFM_MERGE_LEGACY=1, and with the CPU oracle at the
suite's 1e-11."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from test_merge_rowmajor import _geometric_k, _model_passes  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-11
W, G = 70, 20


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


def _parity_table(L, S, G=G, seed=0):
    """k (W, G, L, S) and amounts (S, L): even wavenumbers ten decades between consecutive gases, odd ones equal magnitudes;
    the amounts differ by two decades at most, so eight remain"""
    rng = np.random.default_rng(1000 * L + 10 * S + G + seed)
    far = _geometric_k(rng, W, G, L, S, [-10.0 * s for s in range(S)])
    near = _geometric_k(rng, W, G, L, S, np.zeros(S))
    k = np.where((np.arange(W) % 2 == 0)[:, None, None, None], far, near)
    return k, 10.0 ** rng.uniform(19, 21, (S, L))


def _confirm_by_the_model(oracle, delg, k, amount, rows):
    """the model's verdict at the given rows: every lane of an even wavenumber passes every merge, none of an odd one any"""
    ok = _model_passes(oracle, delg, np.ascontiguousarray(k[:, :, rows, :]), np.ascontiguousarray(amount[:, rows]))
    assert ok[:, 0::2].all() and not ok[:, 1::2].any()


def _call(eng, delg, k, amount):
    tau = eng.k_overlap(delg, k, amount)
    return tau, eng.last_merge_rowmajor(), eng.last_merge_order()


def _other_ways(eng, oracle, delg, k, amount, taus):
    """every result of the default launches against the launch in wavenumber order, the walk off, no trim and the oracle; none
    of the three applies an order, and none of them touches the bytes the default launches keep"""
    for name, env in (("order off", dict(ANSFM_MERGE_ORDER="0")), ("walk off", dict(ANSFM_MERGE_ROWMAJOR="0")),
                      ("legacy", dict(ANSFM_MERGE_LEGACY="1"))):
        with _env(**env):
            other = eng.k_overlap(delg, k, amount)
            assert eng.last_merge_order() == (False, 0), name
        for i, tau in enumerate(taus):
            assert np.array_equal(tau, other), f"call {i + 1} / {name} differ"
    np.testing.assert_allclose(taus[0], oracle.k_overlap(delg, k, amount), rtol=RTOL, atol=0)


@pytest.mark.parametrize("S", [2, 8])
def test_two_wavenumbers_per_tile(eng, oracle, S):
    """L = 32: a tile is two neighbouring positions of the block's order.  First call, wavenumber order: every real tile holds
    an even and an odd wavenumber and nothing walks.  Second call: the odd wavenumbers (byte 0) come first, then the even ones,
    so the full block's 32 tiles are 16 pure odd and 16 pure even ones and exactly half of its (wave, merge) pairs walk; the
    six real wavenumbers of the second block are handed out 65, 67 | 69, 64 | 66, 68, of which the last tile walks."""
    L = 32
    delg = _delg(G)
    k, amount = _parity_table(L, S)
    _confirm_by_the_model(oracle, delg, k, amount, np.arange(L))
    merged = (32 + 3) * (S - 1)                     # the tiles with a real cell, each merge of them
    with _env(ANSFM_MERGE_ORDER="", ANSFM_MERGE_ROWMAJOR="", ANSFM_MERGE_LANES=""):
        tau1, counts1, order1 = _call(eng, delg, k, amount)
        tau2, counts2, order2 = _call(eng, delg, k, amount)
        tau3, counts3, order3 = _call(eng, delg, k, amount)
        print(f"S={S}: walked / merged = {counts1}, {counts2}, {counts3}; order = {order1}, {order2}, {order3}")
        assert order1 == (False, 0)
        assert order2 == (True, 35) and order3 == (True, 35)        # the even real wavenumbers' bytes: 32 + 3
        assert counts1 == (0, merged)
        assert counts2 == ((16 + 1) * (S - 1), merged) and counts3 == counts2
        _other_ways(eng, oracle, delg, k, amount, (tau1, tau2, tau3))


@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("L", [3, 33, 65, 100])
def test_rows_that_do_not_fill_a_tile(eng, oracle, L, S):
    """three calls: the bytes depend on the table alone, so the second and the third call run in the same order and agree; like
    joins like more often than in wavenumber order, never less; which waves merge at all does not change (the pad wavenumbers
    stay behind the real ones)"""
    delg = _delg(G)
    k, amount = _parity_table(L, S)
    _confirm_by_the_model(oracle, delg, k, amount, np.array([0, L // 2, L - 1]))
    with _env(ANSFM_MERGE_ORDER="", ANSFM_MERGE_ROWMAJOR="", ANSFM_MERGE_LANES=""):
        tau1, counts1, order1 = _call(eng, delg, k, amount)
        tau2, counts2, order2 = _call(eng, delg, k, amount)
        tau3, counts3, order3 = _call(eng, delg, k, amount)
        print(f"L={L} S={S}: walked / merged = {counts1}, {counts2}, {counts3}; order = {order1}, {order2}, {order3}")
        assert order1 == (False, 0) and order2 == (True, 35) and order3 == (True, 35)
        assert counts2[0] >= counts1[0] and counts3 == counts2
        assert counts1[1] == counts2[1] > 0
        _other_ways(eng, oracle, delg, k, amount, (tau1, tau2, tau3))


@pytest.mark.parametrize("change", ["L", "S", "G"])
def test_a_change_of_shape_clears_the_bytes(eng, oracle, change):
    """after two calls of one shape, a call of another shape is not applied and counts what a fresh engine counts"""
    import archnemesis_dist_amd as pkg
    L, S, g = 33, 4, G
    L2, S2, g2 = (65 if change == "L" else L), (3 if change == "S" else S), (16 if change == "G" else g)
    k, amount = _parity_table(L, S, g)
    k2, amount2 = _parity_table(L2, S2, g2)
    with _env(ANSFM_MERGE_ORDER="", ANSFM_MERGE_ROWMAJOR="", ANSFM_MERGE_LANES=""):
        _call(eng, _delg(g), k, amount)
        assert _call(eng, _delg(g), k, amount)[2][0]
        tau, counts, order = _call(eng, _delg(g2), k2, amount2)
        assert order == (False, 0)
        tau_b, counts_b, order_b = _call(eng, _delg(g2), k2, amount2)
        assert order_b[0] and counts_b[0] >= counts[0]
        fresh = pkg.AnsfmEngine(0)
        try:
            tau_f, counts_f, order_f = _call(fresh, _delg(g2), k2, amount2)
        finally:
            fresh.close()
    assert order_f == (False, 0) and counts == counts_f, (counts, counts_f)
    assert np.array_equal(tau, tau_f) and np.array_equal(tau, tau_b)


def _fused_case(S=3, L=33, n=3, NP=4, NT=3):
    from archnemesis_dist_amd import synthetic as syn
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=21)
    K[0::2] *= 10.0 ** (-10.0 * np.arange(S))      # even wavenumbers: gases ten decades apart; odd: the generator's magnitudes
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
    table = (K, PRESS, TEMP, WAVE, _delg(G))
    args = (0, lp, lt, am, cont, NLAYIN, LAYINC, SCALE, EMTEMP, np.full(n, -1.0))
    return table, args


@pytest.mark.parametrize("dedup", [True, False])
def test_fused_batch_from_the_table(eng, oracle, dedup):
    """the table path (not FROM_K), three models of 33 layers with and without layer de-duplication, run twice: the second call
    is applied, the spectra are those of the first and of ANSFM_MERGE_ORDER=0 bit for bit; an upload of the same table again
    starts over, with the counts of the first call"""
    table, args = _fused_case()
    eng.upload_ktable(*table)
    eng.set_layer_dedup(dedup)
    try:
        with _env(ANSFM_MERGE_ORDER="", ANSFM_MERGE_ROWMAJOR="", ANSFM_MERGE_LANES=""):
            spec1 = eng.cirsrad_ck_thermal(*args)
            counts1, order1 = eng.last_merge_rowmajor(), eng.last_merge_order()
            spec2 = eng.cirsrad_ck_thermal(*args)
            counts2, order2 = eng.last_merge_rowmajor(), eng.last_merge_order()
            with _env(ANSFM_MERGE_ORDER="0"):
                spec0 = eng.cirsrad_ck_thermal(*args)
                assert eng.last_merge_order() == (False, 0) and eng.last_merge_rowmajor() == counts1
            eng.upload_ktable(*table)
            spec3 = eng.cirsrad_ck_thermal(*args)
            counts3, order3 = eng.last_merge_rowmajor(), eng.last_merge_order()
    finally:
        eng.set_layer_dedup(True)
    print(f"dedup={dedup}: walked / merged = {counts1}, {counts2}, {counts3}; order = {order1}, {order2}, {order3}")
    assert not order1[0] and order2[0] and order2[1] > 0 and order3 == (False, 0)
    assert counts2[0] >= counts1[0] and counts2[1] == counts1[1] and counts3 == counts1
    for other in (spec2, spec0, spec3):
        assert np.array_equal(spec1, other)
    K, PRESS, TEMP, WAVE, delg = table
    _, lp, lt, am, cont, NLAYIN, LAYINC, SCALE, EMTEMP, _ = args
    ref = oracle.cirsrad_ck_thermal(0, K, PRESS, TEMP, WAVE, delg, lp[1], lt[1], am[1], cont[1], NLAYIN, LAYINC, SCALE, EMTEMP[1], -1.0)
    np.testing.assert_allclose(spec1[1], ref, rtol=RTOL, atol=0)


@pytest.mark.parametrize("way", ["pairs", "wavenumbers", "float64 weights", "short list"])
def test_launches_that_do_not_qualify(eng, oracle, way):
    """the other lane mappings, float64 weights (no weight table, no walk) and G = 10 (a head list of 10 entries: the order
    is for lists of 16 and more): never applied, nothing kept, results unchanged"""
    L, S = {"pairs": 33, "wavenumbers": 34, "float64 weights": 35, "short list": 36}[way], 5      # shapes no other launch of this module has
    f32 = way != "float64 weights"
    if way == "short list":
        delg = _delg(10)
        k, amount = _parity_table(L, S, 10, seed=3)
        with _env(ANSFM_MERGE_ORDER="", ANSFM_MERGE_ROWMAJOR="", ANSFM_MERGE_LANES=""):
            tau1, counts1, order1 = _call(eng, delg, k, amount)
            tau2, counts2, order2 = _call(eng, delg, k, amount)
        assert order1 == (False, 0) and order2 == (False, 0)
        assert counts1 == counts2 and np.array_equal(tau1, tau2)
        np.testing.assert_allclose(tau1, oracle.k_overlap(delg, k, amount), rtol=RTOL, atol=0)
        return
    delg = _delg(G, f32)
    k, amount = _parity_table(L, S, seed=3)
    with _env(ANSFM_MERGE_ORDER="", ANSFM_MERGE_ROWMAJOR="", ANSFM_MERGE_LANES="" if not f32 else way):
        tau1, counts1, order1 = _call(eng, delg, k, amount)
        tau2, counts2, order2 = _call(eng, delg, k, amount)
    assert order1 == (False, 0) and order2 == (False, 0)
    assert counts1 == counts2 and np.array_equal(tau1, tau2)
    np.testing.assert_allclose(tau1, oracle.k_overlap(delg, k, amount), rtol=RTOL, atol=0)
    if f32:                                         # the library's own launch of the same table: the same doubles
        with _env(ANSFM_MERGE_ORDER="", ANSFM_MERGE_ROWMAJOR="", ANSFM_MERGE_LANES=""):
            own = [_call(eng, delg, k, amount) for _ in range(2)]
        assert [o[2][0] for o in own] == [False, True]
        assert np.array_equal(own[0][0], tau1) and np.array_equal(own[1][0], tau1)
