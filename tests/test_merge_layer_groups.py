"""The forward merge kernel with a wave's lanes grouped over rows (LaneRow): the library as it launches by
default (lanes grouped over rows), with ANSFM_MERGE_LANES=wavenumbers (64 wavenumbers of one row per wave) and without any trim
(ANSFM_MERGE_LEGACY=1), all bit for bit, and against the CPU oracle at the suite's 1e-11.  The default run must report bit 32 of
ansfm_last_merge_launch's trims, the others must not.  Shapes: one row (every tile runs over wavenumber-group seams, plus pad
lanes); fewer rows than a tile holds; a row axis that ends in a group of one row; fewer cells than a wave; a batch of models
with and without layer de-duplication; and the row count of the benchmark, where a tile crosses into the next wavenumber
group at row 100."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from test_merge_trim import _sweep_k  # noqa: E402  (random; flat to 1e-9; leading zeros; a zero gas in some cells)
from test_merge_weight_table import _cirsrad_case as _wt_cirsrad_case  # noqa: E402  (a k-table of those four kinds)

pytestmark = pytest.mark.gpu

RTOL = 1e-11
G_SWEEP = [8, 10, 12, 16, 20, 32]
LANE_ROWS = 32                                     # bit of ansfm_last_merge_launch's trims
SHAPES = [(70, 1), (64, 3), (136, 33), (6, 5)]     # (W, L)


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


def _relmax(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def _three_ways(eng, run):
    """run() as the library launches it by default (grouped over rows), over wavenumbers and without the trims: the three
    results, after the launch reports are checked"""
    with _env(ANSFM_MERGE_LANES=""):               # not "wavenumbers": the library's own choice
        rows = run()
        rows_launch = eng.last_merge_launch()
    with _env(ANSFM_MERGE_LANES="wavenumbers"):
        waves = run()
        waves_launch = eng.last_merge_launch()
    with _env(ANSFM_MERGE_LEGACY="1"):
        legacy = run()
        legacy_launch = eng.last_merge_launch()
    assert rows_launch[1] & LANE_ROWS and rows_launch[1] & 8 and rows_launch[1] & 16, rows_launch
    assert waves_launch[1] != 0 and not waves_launch[1] & LANE_ROWS, waves_launch
    assert waves_launch == (rows_launch[0], rows_launch[1] & ~LANE_ROWS)
    assert legacy_launch == (1, 0), legacy_launch
    return rows, waves, legacy


def _same(a, b):
    if isinstance(a, tuple):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def _delg(G, f32):
    from archnemesis_dist_amd import synthetic as syn
    return syn.gauss_legendre_01(G, f32)[1]


def test_default_mapping_is_reported(eng):
    """Without ANSFM_MERGE_LANES the launch groups the lanes over rows and says so; with "wavenumbers" it does not."""
    rng = np.random.default_rng(1)
    delg = _delg(20, True)
    k = _sweep_k(rng, 70, 20, 3, 3)
    amount = 10.0 ** rng.uniform(19, 22, (3, 3))
    with _env(ANSFM_MERGE_LANES=""):               # not "wavenumbers": the library's own choice
        tau = eng.k_overlap(delg, k, amount)
        assert eng.last_merge_launch()[1] & LANE_ROWS
    with _env(ANSFM_MERGE_LANES="wavenumbers"):
        other = eng.k_overlap(delg, k, amount)
        assert not eng.last_merge_launch()[1] & LANE_ROWS
    assert np.array_equal(tau, other)


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"W{s[0]}L{s[1]}")
@pytest.mark.parametrize("G", G_SWEEP)
def test_k_overlap_layer_groups(eng, oracle, G, shape, f32):
    W, L = shape
    S = 3
    rng = np.random.default_rng(8000 + 100 * G + 10 * W + L)
    delg = _delg(G, f32)
    k = _sweep_k(rng, W, G, L, S)
    amount = 10.0 ** rng.uniform(19, 22, (S, L))
    rows, waves, legacy = _three_ways(eng, lambda: eng.k_overlap(delg, k, amount))
    ref = oracle.k_overlap(delg, k, amount)
    print(f"k_overlap G={G} W={W} L={L} f32={f32}: rows vs oracle {_relmax(rows, ref):.3e}, bits equal "
          f"{np.array_equal(rows, waves)} / {np.array_equal(rows, legacy)}")
    assert np.array_equal(rows, waves) and np.array_equal(rows, legacy)
    np.testing.assert_allclose(rows, ref, rtol=RTOL, atol=0)


def _cirsrad_case(rng, W, G, S, L, f32, positive, NP=3, NT=2):
    from archnemesis_dist_amd import synthetic as syn
    delg = _delg(G, f32)
    PRESS, TEMP, Kpos = syn.synth_ktable(W, G, NP, NT, S, seed=5 + W + L)
    K = Kpos if positive else np.ascontiguousarray(_sweep_k(rng, W, G, NP * NT, S).reshape(W, G, NP, NT, S))
    WAVE = 250.0 + 0.5 * np.arange(W)
    atm = syn.synth_atmosphere(max(L, 2), S, seed=11 + L)      # the generator needs two layers: L = 1 takes the lower one
    atm = {key: np.ascontiguousarray(v[..., :L]) for key, v in atm.items()}
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


def _check_cirsrad(eng, oracle, c, positive, label, against_oracle=True):
    """One fused forward model three ways: spectrum and gas opacities bit for bit, and (against_oracle) both at 1e-11"""
    eng.upload_ktable(c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"])
    assert eng.ktable_info()[1]                    # monotone: the fast path
    assert eng.ktable_has_boxed() is (not positive)
    rows, waves, legacy = _three_ways(eng, lambda: _run_cirsrad(eng, c))
    a = c["atm"]
    ref, rtg = oracle.cirsrad_ck_thermal(0, c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"], a["lay_press_pa"][0],
                                         a["lay_temp"][0], a["amount"][0], c["cont"][0], c["NLAYIN"], c["LAYINC"],
                                         c["SCALE"], c["EMTEMP"], -1.0, return_taugas=True)
    ref = np.squeeze(ref)
    err = np.abs(rows[1] - rtg) / np.maximum(np.abs(rtg), 1e-300)
    print(f"cirsrad {label} positive={positive}: taugas {err.max():.3e} (worst (w, g, l) = "
          f"{tuple(int(i) for i in np.unravel_index(np.argmax(err), err.shape))}, {int(np.sum(err > RTOL))} above {RTOL}), spectrum "
          f"{_relmax(rows[0], ref):.3e} vs oracle, bits equal {_same(rows, waves)} / {_same(rows, legacy)}")
    assert _same(rows, waves) and _same(rows, legacy)
    if against_oracle:
        np.testing.assert_allclose(rows[1], rtg, rtol=RTOL, atol=0)
        np.testing.assert_allclose(rows[0], ref, rtol=RTOL, atol=0)


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("G", G_SWEEP)
def test_cirsrad_layer_groups(eng, oracle, G, f32):
    """The fused forward model at all four shapes on a table with boxed entries (the four kinds of _sweep_k along the
    wavenumber axis) and on an all-positive one (read without the box tests): the three ways bit for bit in every case.

    Against the oracle at 1e-11: every case but the boxed table with float64 weights at W = 70, L = 1.  There a column
    whose low g-ordinates are zero jumps by five decades or more, the bins below the jump hold a sliver of the first large
    element, and the reference's own frac, a quotient of differences of cumulative float64 sums, is not good to 1e-11: at
    G = 20 the oracle is 1.7e-10 and 3.3e-10 away from the same rebinning in exact rational arithmetic
    (tools/experiments/r08_oracle_conditioning_probe.py, CPU only) and the kernel, all three ways alike, 4.7e-11 from the
    oracle.  The deviation is printed there.  The table of tests/test_merge_weight_table.py::test_cirsrad_old_and_new_paths
    (boxed, float64 weights, W = 136, L = 3, S = 8) is run the three ways and against the oracle as well."""
    rng = np.random.default_rng(9000 + G)
    for W, L in SHAPES:
        for positive in (False, True):
            c = _cirsrad_case(rng, W, G, 3, L, f32, positive)
            _check_cirsrad(eng, oracle, c, positive, f"G={G} f32={f32} W={W} L={L}", against_oracle=f32 or positive or L != 1)
    if not f32:
        S = 8
        rng = np.random.default_rng(9100 + 10 * G + S)             # the existing test's draws, in its order
        _wt_cirsrad_case(rng, 136, G, S, 3, f32, True)
        c = _wt_cirsrad_case(rng, 136, G, S, 3, f32, False)
        _check_cirsrad(eng, oracle, c, False, f"G={G} f32={f32} W=136 L=3 S=8 (weight-table test's table)")


@pytest.mark.parametrize("dedup", [True, False])
def test_batch_of_models_with_shared_rows(eng, oracle, dedup):
    """Three models at L = 4 that differ from the first in one layer each: with the de-duplication the merge sees the
    distinct rows only, without it all twelve."""
    from archnemesis_dist_amd import synthetic as syn
    W, G, S, L, NP, NT, n = 70, 20, 3, 4, 4, 3, 3
    delg = _delg(G, True)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=21)
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
        rows, waves, legacy = _three_ways(eng, run)
        computed, total = eng.last_layer_rows()
    finally:
        eng.set_layer_dedup(True)
    print(f"dedup={dedup}: rows computed {computed} of {total}")
    assert total == n * L and (computed < total if dedup else computed == total)
    assert np.array_equal(rows, waves) and np.array_equal(rows, legacy)
    for i in range(n):
        ref = oracle.cirsrad_ck_thermal(0, K, PRESS, TEMP, WAVE, delg, lp[i], lt[i], am[i], cont[i], NLAYIN, LAYINC, SCALE,
                                        EMTEMP[i], -1.0)
        np.testing.assert_allclose(rows[i], ref, rtol=RTOL, atol=0)


def test_device_entry_at_the_benchmark_row_count(eng, oracle):
    """cirsrad_ck_thermal_dev at W = 136, L = 100, S = 8, G = 20: tiles of 32 or fewer rows do not divide 100, so tiles cross
    into the next wavenumber group."""
    import torch
    from archnemesis_dist_amd import synthetic as syn
    W, G, S, L, NP, NT = 136, 20, 8, 100, 4, 3
    delg = _delg(G, True)
    PRESS, TEMP, K = syn.synth_ktable(W, G, NP, NT, S, seed=31)
    WAVE = 300.0 + np.arange(W) * 1.0
    atm = syn.synth_atmosphere(L, S, seed=32)
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, 10.0)
    cont = syn.synth_continuum(W, L)
    EMTEMP = atm["lay_temp"][:, LAYINC[:, 0]][:, :, None]
    eng.upload_ktable(K, PRESS, TEMP, WAVE, delg)
    dev = torch.device("cuda:0")
    td = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    d = [td(atm["lay_press_pa"][0]), td(atm["lay_temp"][0]), td(atm["amount"][0]), td(cont), td(NLAYIN, torch.int32),
         td(LAYINC, torch.int32), td(SCALE), td(EMTEMP[0]), td(np.full(1, -1.0))]
    out = torch.empty((1, W, 1), dtype=torch.float64, device=dev)

    def run():
        eng.cirsrad_ck_thermal_dev(0, 1, L, d[0], d[1], d[2], d[3], 1, LAYINC.shape[0], d[4], d[5], d[6], d[7], d[8], None,
                                   None, None, None, None, None, out)
        torch.cuda.synchronize()
        return out.cpu().numpy()[0, :, 0].copy(), eng.get_taugas(L, 0)

    rows, waves, legacy = _three_ways(eng, run)
    ref, rtg = oracle.cirsrad_ck_thermal(0, K, PRESS, TEMP, WAVE, delg, atm["lay_press_pa"][0], atm["lay_temp"][0],
                                         atm["amount"][0], cont[0], NLAYIN, LAYINC, SCALE, EMTEMP[0], -1.0, return_taugas=True)
    print(f"device entry L=100: taugas {_relmax(rows[1], rtg):.3e}, spectrum {_relmax(rows[0], np.squeeze(ref)):.3e} vs oracle")
    assert _same(rows, waves) and _same(rows, legacy)
    np.testing.assert_allclose(rows[1], rtg, rtol=RTOL, atol=0)
    np.testing.assert_allclose(rows[0], np.squeeze(ref), rtol=RTOL, atol=0)
