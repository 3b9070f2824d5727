"""The forward merge reading the k-table from its g-fastest copy (lnKg[NP][NT][S][Wpad][Gs], built by
k_table_gfast at every k-table upload unless ANSFM_TABLE_GFAST=0, read by load_gas_rows as 16-byte pairs of ordinates).  Every case runs
the fused thermal call three ways -- as the library launches it, with ANSFM_TABLE_LAYOUT=wave (the reads of lnK) and with
ANSFM_MERGE_LEGACY=1 (no trim) -- and compares the gas opacities tau and the spectra bit for bit; the first is also compared
with the CPU oracle at the 1e-11 of tests/test_merge_one_wavenumber.py.  ansfm_ktable_gfast and
ansfm_last_merge_table_layout must report which path ran."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-11
NP, NT = 5, 4


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


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


def _copy_bytes(W, G, S, np_=NP, nt=NT):
    wpad, gs = (W + 63) // 64 * 64, (G + 1) // 2 * 2
    return np_ * nt * S * wpad * gs * 8


def _case(W, L, G, S, n=1, seed=0, f32=True, boxed=False):
    """A synthetic table and n states of L layers; states 1 .. n - 1 differ from state 0 in one layer each"""
    from archnemesis_dist_amd import synthetic as syn
    delg = syn.gauss_legendre_01(G, as_float32=f32)[1]
    if f32:
        delg = delg.astype(np.float32)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=1000 + seed, zero_low_g=boxed)
    WAVE = 300.0 + np.arange(W) * 1.0
    atm = syn.synth_atmosphere(max(L, 2), S, seed=2000 + seed)
    lp = np.repeat(atm["lay_press_pa"][:1, :L], n, axis=0)
    lt = np.repeat(atm["lay_temp"][:1, :L], n, axis=0)
    am = np.repeat(atm["amount"][:1, :, :L], n, axis=0)
    for i in range(1, n):
        lt[i, i % L] += 3.0 * i
        am[i, :, i % L] *= 1.0 + 0.25 * i
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, 10.0)
    cont = np.repeat(syn.synth_continuum(W, L)[:1], n, axis=0)
    EMTEMP = lt[:, LAYINC[:, 0]][:, :, None]
    return dict(K=K, PRESS=PRESS, TEMP=TEMP, WAVE=WAVE, delg=delg, lp=lp, lt=lt, am=am, cont=cont, NLAYIN=NLAYIN,
                LAYINC=LAYINC, SCALE=SCALE, EMTEMP=EMTEMP, n=n, L=L)


def _upload(eng, c, gfast="1"):
    with _env(ANSFM_TABLE_GFAST=gfast):
        eng.upload_ktable(c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"])


def _run(eng, c):
    """(spectra, tau of every state) of the fused thermal call"""
    n, L = c["n"], c["L"]
    spec = eng.cirsrad_ck_thermal(0, c["lp"], c["lt"], c["am"], c["cont"], c["NLAYIN"], c["LAYINC"], c["SCALE"], c["EMTEMP"],
                                  np.full(n, -1.0))
    return (np.array(spec),) + tuple(eng.get_taugas(L, m) for m in range(n))


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _three_ways(eng, c, copy=True, width=1):
    """The default launch, ANSFM_TABLE_LAYOUT=wave and ANSFM_MERGE_LEGACY=1, bit for bit; returns the first.  copy: the context
    holds the g-fastest copy, so the default launch must report its reads and the other two must not."""
    res = _run(eng, c)
    assert eng.last_merge_table_layout() is copy
    assert eng.last_merge_group_width() == width
    with _env(ANSFM_TABLE_LAYOUT="wave"):
        wave = _run(eng, c)
        assert eng.last_merge_table_layout() is False
        assert eng.last_merge_group_width() == width
    with _env(ANSFM_MERGE_LEGACY="1"):
        legacy = _run(eng, c)
        assert eng.last_merge_table_layout() is False
        assert eng.last_merge_launch() == (1, 0)
    assert _same(res, wave), "g-fastest / wave-fastest reads differ"
    assert _same(res, legacy), "g-fastest reads / legacy differ"
    return res


def _against_oracle(oracle, c, res):
    worst = 0.0
    for m in range(c["n"]):
        spec, tau = oracle.cirsrad_ck_thermal(0, c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"], c["lp"][m], c["lt"][m],
                                              c["am"][m], c["cont"][m], c["NLAYIN"], c["LAYINC"], c["SCALE"], c["EMTEMP"][m], -1.0,
                                              return_taugas=True)
        worst = max(worst, float(np.max(np.abs(res[1 + m] - tau) / np.maximum(np.abs(tau), 1e-300))))
        np.testing.assert_allclose(res[1 + m], tau, rtol=RTOL, atol=0)
        np.testing.assert_allclose(res[0][m], spec, rtol=RTOL, atol=0)
    return worst


def _check(eng, oracle, c, width=1):
    W, G, _, _, S = c["K"].shape
    _upload(eng, c)
    assert eng.ktable_gfast() == (True, _copy_bytes(W, G, S))
    res = _three_ways(eng, c, width=width)
    err = _against_oracle(oracle, c, res)
    print(f"W={W} L={c['L']} G={G} S={S} n={c['n']}: tau vs oracle {err:.3e}")
    assert res[1].max() > 0
    return res


@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("shape", [(70, 3), (2, 32), (70, 1), (70, 33), (70, 64), (70, 100)], ids=lambda s: f"W{s[0]}L{s[1]}")
def test_shapes(eng, oracle, shape, S):
    """G = 20: pad lanes in the last block (W = 70, Wpad = 128); fewer cells than a wave (W = 2, L = 32); one row; tiles that
    run over the wavenumber seam (3, 33, 100 rows); exactly one tile per wavenumber (64 rows).  Two and eight gases."""
    W, L = shape
    _check(eng, oracle, _case(W, L, 20, S, seed=W + L + S))


@pytest.mark.parametrize("G", [7, 10, 12, 32])
def test_ordinate_counts(eng, oracle, G):
    """G = 7: odd, so the padded stride 8 and a last pair whose second ordinate is the pad; 10: one batch exactly; 12: list
    length 16, a second batch of one pair and four clamped ones; 32: four batches, the last of one pair."""
    _check(eng, oracle, _case(70, 3, G, 4, seed=G))


def test_boxed_table(eng, oracle):
    """Entries <= 0 (stored boxed): the loads with the box tests, NOBOX off"""
    c = _case(70, 33, 20, 3, seed=5, boxed=True)
    _check(eng, oracle, c)
    assert eng.ktable_has_boxed()


@pytest.mark.parametrize("L", [3, 65])
def test_float64_weights(eng, oracle, L):
    """float64 weights: the instantiations without the weight table read the copy as well"""
    c = _case(70, L, 20, 4, seed=6, f32=False)
    _check(eng, oracle, c)
    _run(eng, c)
    assert eng.last_merge_table_layout() and not eng.last_merge_launch()[1] & 1


@pytest.mark.parametrize("dedup", [True, False])
def test_batch(eng, oracle, dedup):
    """Three states that differ from the first in one layer each, with and without layer de-duplication"""
    c = _case(70, 4, 20, 3, n=3, seed=7)
    eng.set_layer_dedup(dedup)
    try:
        _check(eng, oracle, c)
        computed, total = eng.last_layer_rows()
    finally:
        eng.set_layer_dedup(True)
    assert total == 12 and (computed < total if dedup else computed == total)


@pytest.mark.parametrize("G", [20, 7])
def test_pairs(eng, oracle, G):
    """ANSFM_MERGE_LANES=pairs: two wavenumbers x 32 rows per wave on the same reads"""
    c = _case(70, 33, G, 3, seed=8)
    one = _check(eng, oracle, c)
    with _env(ANSFM_MERGE_LANES="pairs"):
        two = _check(eng, oracle, c, width=2)
    assert _same(one, two)


def test_second_context_holds_a_slice(eng, oracle):
    """A second context with wavenumbers 10 .. 49 of the same table: its own copy, the same opacities"""
    import archnemesis_dist_amd as pkg
    c = _case(70, 33, 20, 3, seed=9)
    full = _check(eng, oracle, c)
    sl = slice(10, 50)
    c2 = dict(c, K=np.ascontiguousarray(c["K"][sl]), WAVE=c["WAVE"][sl], cont=np.ascontiguousarray(c["cont"][:, sl]))
    e2 = pkg.AnsfmEngine(0)
    try:
        part = _check(e2, oracle, c2)
        assert e2.ktable_gfast() == (True, _copy_bytes(40, 20, 3))
    finally:
        e2.close()
    assert np.array_equal(part[1], full[1][sl])
    assert eng.ktable_gfast() == (True, _copy_bytes(70, 20, 3))


def test_kta_files(eng, golden_dir):
    """The .kta reader builds the copy too: equal to the wave-fastest reads and to the upload of the arrays the reference read"""
    import archnemesis_dist_amd as pkg
    from archnemesis_dist_amd import synthetic as syn
    z = np.load(os.path.join(golden_dir, "kta_read.npz"))
    paths = [os.path.join(golden_dir, "kta", f"uni_gas{gi}.kta") for gi in range(2)]
    lo, hi = z["uni0_all_range"]
    K = np.stack([z[f"uni{gi}_all_k"] for gi in range(2)], axis=-1)
    W, G, np_, nt, S = K.shape
    L = 5
    atm = syn.synth_atmosphere(L, S, seed=3)
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, 10.0)
    c = dict(lp=atm["lay_press_pa"], lt=atm["lay_temp"], am=atm["amount"], cont=syn.synth_continuum(W, L), NLAYIN=NLAYIN,
             LAYINC=LAYINC, SCALE=SCALE, EMTEMP=atm["lay_temp"][:, LAYINC[:, 0]][:, :, None], n=1, L=L)
    e1 = pkg.AnsfmEngine(0)
    try:
        with _env(ANSFM_TABLE_GFAST="1"):
            e1.upload_ktable_files(paths, lo, hi)
        assert e1.ktable_gfast() == (G >= 2, _copy_bytes(W, G, S, np_, nt) if G >= 2 else 0)
        files = _three_ways(e1, c, copy=G >= 2)
    finally:
        e1.close()
    with _env(ANSFM_TABLE_GFAST="1"):
        eng.upload_ktable(K, z["uni0_head_presslevels"], z["uni0_head_templevels"], z["uni0_all_wave"], z["uni0_head_del_g"])
    arrays = _three_ways(eng, c, copy=G >= 2)
    assert _same(files, arrays)
    assert files[1].max() > 0


def test_switched_off_and_replaced(eng, oracle):
    """ANSFM_TABLE_GFAST=0 at the upload: no copy, the old reads, equal results.  A later upload of a smaller table with the
    switch on builds that table's copy; one with the switch off drops it again."""
    c = _case(70, 33, 20, 3, seed=10)
    on = _check(eng, oracle, c)
    _upload(eng, c, gfast="0")
    assert eng.ktable_gfast() == (False, 0)
    off = _three_ways(eng, c, copy=False)
    assert _same(on, off)
    _against_oracle(oracle, c, off)
    small = _case(40, 3, 12, 2, seed=11)
    _check(eng, oracle, small)
    assert eng.ktable_gfast() == (True, _copy_bytes(40, 12, 2))
    _upload(eng, small, gfast="0")
    assert eng.ktable_gfast() == (False, 0)
    assert _same(_three_ways(eng, small, copy=False), _run(eng, small))


def test_one_ordinate_has_no_copy(eng):
    """G = 1 (and with it every LBL table) is never copied"""
    c = _case(70, 3, 1, 2, seed=12)
    _upload(eng, c)
    assert eng.ktable_gfast() == (False, 0)
