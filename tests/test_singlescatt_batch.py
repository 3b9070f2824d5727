"""ansfm_cirsrad_ck_singlescatt_batch: CIRSrad's single-scattering branch (ISCAT = 3) for the states of a numerical Jacobian in
one call.  The batch against separate single-model calls bit for bit (gas-opacity de-duplication and the prefix records of
state 0 on and off; sorted, g-scrambled and line-by-line tables; a caller's stream), against the reference's recipe on the CPU
oracle, against the reference's own jacobian_nemesis run (tests/golden/jacobian_ss.npz, tools/golden/gen_golden_jacobian_ss.py),
and at C2 width."""
import os

import numpy as np
import pytest

import singlescatt_cases as sc


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


def _states(kind, tsurf0, tsurf_other, W=100, G=10, S=3, L=9):
    t = sc.synthetic_table(kind, W, G, S)
    b = sc.base_state(W, S, L)
    return t, b, sc.jacobian_like_states(b, tsurf0, tsurf_other)


def _check_batch_equals_singles(eng, b, s, dedup):
    n, L = s["lp"].shape
    eng.set_layer_dedup(dedup)
    try:
        got = sc.batch_call(eng, b, s)
        rows, total = eng.last_layer_rows()
        shared = eng.last_rt_shared()
    finally:
        eng.set_layer_dedup(True)
    assert got.shape == (n, b["xfac"].size, 2) and total == n * L
    if dedup:
        # state 0's L rows, one more for the temperature state and one for the gas-amount state
        assert rows == L + 2 and rows < n * L and shared
    else:
        assert rows == n * L and not shared
    for m in range(n):
        one = sc.single_call(eng, b, s, m)
        assert np.array_equal(one, got[m]), (m, float(np.max(np.abs(one - got[m]) / np.abs(one))))
    assert np.array_equal(got[6], got[0])                       # the state that differs in nothing
    for m in range(1, 6):                                       # ... and every other one does differ, in the path it touches
        assert not np.array_equal(got[m], got[0]), m
    assert np.array_equal(got[4][:, 0], got[0][:, 0]) and not np.array_equal(got[4][:, 1], got[0][:, 1])   # phase of path 1 only
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("dedup", [True, False], ids=["shared", "unshared"])
@pytest.mark.parametrize("kind", ["sorted", "scrambled", "lbl"])
@pytest.mark.parametrize("tsurf", [(-1.0, 240.0), (260.0, -1.0)], ids=["tsurf_neg", "tsurf_pos"])
def test_batch_equals_separate_calls_bit_for_bit(eng, kind, dedup, tsurf):
    """State 0 and six states that differ from it in one layer's temperature, one gas amount, one layer's scattering opacity,
    one path's phase function, TSURF, and nothing: the batched call returns what seven single-model calls return, to the last
    bit, with the sharing (distinct gas-opacity rows, state 0's prefix records) and with ansfm_set_layer_dedup(ctx, 0)."""
    t, b, s = _states(kind, *tsurf)
    sc.upload(eng, t)
    if kind != "lbl":
        assert eng.ktable_info()[1] is (kind == "sorted")
    _check_batch_equals_singles(eng, b, s, dedup)


@pytest.mark.gpu
def test_batch_on_the_callers_stream(eng):
    """The same batch with the engine on a torch stream that is not the default one."""
    import torch
    t, b, s = _states("sorted", -1.0, 240.0)
    sc.upload(eng, t)
    ref = _check_batch_equals_singles(eng, b, s, True)
    side = torch.cuda.Stream(device=0)
    try:
        with torch.cuda.stream(side):
            eng.set_stream(side.cuda_stream)
            got = sc.batch_call(eng, b, s)
            assert eng.last_rt_shared()
    finally:
        eng.set_stream(None)
    assert np.array_equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("tsurf", [(-1.0, 240.0), (260.0, -1.0)], ids=["tsurf_neg", "tsurf_pos"])
def test_batch_vs_oracle_chain(eng, oracle, tsurf):
    """Every state of the batch against the reference's recipe on the oracle's pieces (calc_k -> k_overlap -> omega ->
    calc_singlescatt_plane_spectrum per path -> g-quadrature), at the tolerance the single-model test holds: 1e-11."""
    t, b, s = _states("sorted", *tsurf)
    sc.upload(eng, t)
    got = sc.batch_call(eng, b, s)
    assert eng.last_rt_shared()
    omega_max = 0.0
    for m in range(got.shape[0]):
        ref = sc.oracle_chain(oracle, t, 0, s["lp"][m], s["lt"][m], s["am"][m], s["cont"][m], s["sca"][m], s["phase"][m], b["NLAYIN"],
                              b["LAYINC"], s["SCALE"][m], s["EMTEMP"][m], float(s["TSURF"][m]), b["EMIS"], b["BRDF"], b["SOLF"], b["sol"],
                              b["emi"], xfac=b["xfac"])
        print("state %d: max rel err vs the oracle chain %.3e" % (m, float(np.max(np.abs(got[m] - ref) / np.abs(ref)))))
        np.testing.assert_allclose(got[m], ref, rtol=1e-11)
    k = oracle.calc_k(t["K"], t["PRESS"], t["TEMP"], b["lp"] / 101325.0, b["lt"])
    tautot = oracle.k_overlap(t["delg"], k, b["am"]) + b["cont"][:, None, :]
    omega_max = float(np.max(b["sca"][:, None, :] / tautot))
    assert 0.8 < omega_max < 1.0, omega_max                     # the albedo does reach about 0.9


@pytest.mark.gpu
def test_replay_of_the_reference_singlescatt_jacobian(eng, golden_dir):
    """The nine forward models of the reference's jacobian_nemesis run with ISCAT = 3 as ONE batched call: every spectrum
    within 2e-7 of the reference's SPECOUT (the float32 logarithm of the table grids), KK formed with
    finite_difference_jacobian within 1e-4 of each column's maximum; the temperature elements re-adjust 13-26 of the 30 layers,
    the aerosol elements change 3-4, so both little and much of state 0 is shared."""
    z = np.load(os.path.join(golden_dir, "jacobian_ss.npz"))
    n, L = z["LAY_PRESS"].shape
    assert n == 9 and int(z["IMOD"][0]) & 1024 and float(np.median(z["SOLAR_SHARE"])) >= 0.1
    sc.upload(eng, sc.fixture_table(z))
    spec = eng.cirsrad_ck_singlescatt_batch(*sc.fixture_batch_args(z))
    rows, total = eng.last_layer_rows()
    print("rows %d of %d, worst spectrum error %.3e" % (rows, total, float(np.max(np.abs(spec - z["SPECOUT"]) / np.abs(z["SPECOUT"])))))
    assert total == n * L and L < rows < total and eng.last_rt_shared()
    np.testing.assert_allclose(spec, z["SPECOUT"], rtol=2e-7)
    YN, KK = sc.kk_from_spectra(z, spec)
    np.testing.assert_allclose(YN, z["YN"], rtol=2e-7)
    sc.assert_kk(KK, z, 1e-4)


@pytest.mark.gpu
def test_batch_at_c2_width(eng):
    """W = 10^4 (157 wavenumber tiles, W not a multiple of 64), L = 100, n = 8 states of a Jacobian: two of the states against
    calls of their own, bit for bit."""
    W, G, S, L, n = 10000, 20, 8, 100, 8
    t = sc.synthetic_table("sorted", W, G, S, NP=6, NT=5)
    b = sc.base_state(W, S, L, seed=7)
    rep = lambda a: np.repeat(np.asarray(a)[None], n, axis=0).copy()
    s = dict(lp=rep(b["lp"]), lt=rep(b["lt"]), am=rep(b["am"]), cont=rep(b["cont"]), sca=rep(b["sca"]), phase=rep(b["phase"]),
             SCALE=rep(b["SCALE"]), TSURF=np.full(n, 180.0))
    for m in range(1, n):                                       # a level's perturbation: a few neighbouring layers each
        lay = 12 * m
        s["lt"][m, lay:lay + 2] *= 1.002
        s["am"][m, :, lay:lay + 3] *= 1.01
        s["sca"][m, :, lay] *= 1.03
        s["cont"][m, :, lay] *= 1.02
        s["phase"][m, m % 2, :, lay + 1] *= 1.04
    s["EMTEMP"] = np.stack([sc.emtemp_of(b, s["lt"][m]) for m in range(n)])
    sc.upload(eng, t)
    got = sc.batch_call(eng, b, s)
    rows, total = eng.last_layer_rows()
    assert total == n * L and rows == L + 3 * (n - 1) and eng.last_rt_shared()
    assert got.shape == (n, W, 2) and np.all(np.isfinite(got))
    for m in (3, n - 1):
        assert np.array_equal(sc.single_call(eng, b, s, m), got[m]), m
        assert not np.array_equal(got[m], got[0])
