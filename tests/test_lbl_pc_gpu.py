"""ansfm_add_pseudo_continuum_monochromatic_absorption and the gas accumulator (ansfm_lbl_accum_*) on the GPU: the reference's
results (tests/golden/lbl_pseudo_continuum.npz, tools/golden/gen_golden_lbl_pc.py) at the tolerances of the line kernel's
tests -- parameters and the spread continuum to rtol 1e-12, spectra to rtol 1e-9 / atol 1e-300, expected zeros exactly zero --
the batch against single calls bit for bit, properties and a window of the NumPy restatement (tests/lbl_pc_cases.py, held to
the reference bit for bit by tests/test_lbl_pc_restatement.py) at 2e5 points x 2000 bins x 4 layers, the accumulator
against host-`out` calls bit for bit, and the argument checks."""
import os

import numpy as np
import pytest

import lbl_pc_cases as pc
from test_lbl_pc_restatement import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return pc.load_golden(os.path.join(golden_dir, "lbl_pseudo_continuum.npz"))


@pytest.mark.parametrize("name", CASES)
def test_golden(eng, golden, name):
    g = golden[name]
    N = g["centers"].shape[0]
    out, store, store_x = g["out0"].copy(), np.full((3, N), np.nan), np.full(N, np.nan)
    eng.add_pseudo_continuum_monochromatic_absorption(*pc.engine_args(g), out, store=store, store_x=store_x,
                                                      n_neighbour_bins=g["n_neighbour_bins"])
    for what, got, ref in (("store", store, g["store"]), ("store_x", store_x, g["store_x"]), ("out", out, g["out"])):
        nz = ref != 0
        print(f"{name}: {what} max rel err {float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]))) if nz.any() else 0.0:.3e}")
    np.testing.assert_allclose(store, g["store"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(store_x, g["store_x"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(out, g["out"], rtol=1e-9, atol=1e-300)
    # exact zeros stay exact zeros: the untouched points, the largest touched point, the bins that do not spread
    assert not np.any(out[g["out"] == 0]) and not np.any(store_x[g["store_x"] == 0])
    changed = np.count_nonzero(out - g["out0"])
    if name in pc.COVERING:
        assert np.count_nonzero(g["out"] - g["out0"]) >= out.size - 1 and changed >= out.size - 1
    if name == "starts_inside":
        assert changed == 0 and not np.any(store_x)


def test_batch_equals_single_calls_bit_for_bit(eng, golden):
    g = dict(golden["jittered"])
    g["t_calc"] = np.array([130.0, 210.0, 295.0]); g["p_calc"] = np.array([0.02, 0.4, 1.3]); g["q_ratio"] = np.array([2.8, 1.5, 1.0])
    N, nw = g["centers"].shape[0], g["wn_grid"].shape[0]
    out, store, store_x = np.zeros((3, nw)), np.zeros((3, 3, N)), np.zeros((3, N))
    eng.add_pseudo_continuum_monochromatic_absorption(*pc.engine_args(g), out, store=store, store_x=store_x)
    assert np.count_nonzero(out) > 0.8 * out.size
    for l in range(3):
        o1, s1, x1 = np.zeros(nw), np.zeros((3, N)), np.zeros(N)
        eng.add_pseudo_continuum_monochromatic_absorption(*pc.engine_args(g, l), o1, store=s1, store_x=x1)
        assert np.array_equal(o1, out[l]) and np.array_equal(s1, store[l]) and np.array_equal(x1, store_x[l])
    assert not np.array_equal(out[0], out[1])


def test_size_and_properties(eng):
    d = pc.big_case()
    nw, N, L = d["wn_grid"].shape[0], d["centers"].shape[0], d["t_calc"].shape[0]
    assert (nw, N, L) == (200000, 2000, 4)
    out, store_x = np.zeros((L, nw)), np.zeros((L, N))
    eng.add_pseudo_continuum_monochromatic_absorption(*pc.engine_args(d), out, store_x=store_x)
    # twice the abundance is exactly twice the spectrum: the factor enters every term of the interpolation once
    d2 = dict(d); d2["isotopic_abundance"] = 2.0 * d["isotopic_abundance"]
    out2 = np.zeros((L, nw))
    eng.add_pseudo_continuum_monochromatic_absorption(*pc.engine_args(d2), out2)
    assert np.array_equal(out2, 2.0 * out)
    # the largest touched grid point and everything outside the bins stay zero; every point below is touched
    first, last, jmax, _ = pc.geometry(d["wn_grid"], d["centers"], d["widths"])
    assert first == 0 and last == N and 0 < jmax < nw - 5000
    assert d["wn_grid"][jmax + 1] >= d["centers"][-1] + 0.5 * d["widths"][-1] > d["wn_grid"][jmax]
    assert not np.any(out[:, jmax:]) and np.all(out[:, :jmax] > 0)
    # a window of 2000 grid points against the restatement
    j0 = 123400
    for l in range(L):
        ref = np.zeros(nw)
        _, x = pc.pseudo_continuum_np(*pc.engine_args(d, l), ref, j_from=j0, j_to=j0 + 2000)
        err = float(np.max(np.abs(out[l, j0:j0 + 2000] - ref[j0:j0 + 2000]) / ref[j0:j0 + 2000]))
        print(f"layer {l}: window max rel err {err:.3e}")
        np.testing.assert_allclose(out[l, j0:j0 + 2000], ref[j0:j0 + 2000], rtol=1e-10, atol=0)
        np.testing.assert_allclose(store_x[l], x, rtol=1e-10, atol=0)


def _gas(rng, wn_grid, L):
    """two isotopologues of a synthetic gas: (line arguments, pseudo-continuum arguments) each, from t_ref on"""
    lo, hi = wn_grid[0], wn_grid[-1]
    c2 = pc.C2
    isos = []
    for iso, (ab, mass) in enumerate(((0.98, 28.0), (0.011, 29.0))):
        n = 400
        nu = np.sort(rng.uniform(lo - 30.0, hi + 30.0, n)); sw = 10.0 ** rng.uniform(-25, -20, n); el = rng.uniform(0, 2000, n)
        bp = np.zeros((3, n)); bp[0] = rng.uniform(0.02, 0.1, n); bp[1] = rng.uniform(0.5, 0.8, n); bp[2] = rng.uniform(-0.01, 0.01, n)
        q = np.linspace(2.0, 1.0, L) * (1.0 + 0.1 * iso)
        mmf = np.array([1.0])
        lines = (pc.VOIGT, 296.0, 1.0, q, ab, mass, mmf, bp, nu, sw, el, 1 - np.exp(-c2 * nu / 296.0))
        centers, widths = pc.regular_bins(np.floor(lo) - 10.0, np.ceil(hi) + 10.0, 1.0)
        b = pc.synth_bins(rng, centers, widths, 1)
        cont = (pc.VOIGT, 296.0, 1.0, q, ab, mass, mmf, b["bparams"], centers, widths, b["sw_sum"], b["e_lower"])
        isos.append((lines, cont))
    return isos


def test_accumulator_equals_host_out_calls_bit_for_bit(eng):
    import torch
    rng = np.random.default_rng(5)
    L, nw = 3, 30000
    wn_grid = 2000.0 + 0.004 * np.arange(nw)
    t, p = np.array([150.0, 220.0, 290.0]), np.array([0.01, 0.2, 1.0])
    isos = _gas(rng, wn_grid, L)
    host = np.zeros((L, nw))
    acc = eng.lbl_accumulator(wn_grid, t, p)
    assert not np.any(acc.numpy())
    for lines, cont in isos:
        eng.add_line_set_monochromatic_absorption(wn_grid, lines[0], t, lines[1], p, *lines[2:], host)
        eng.add_pseudo_continuum_monochromatic_absorption(wn_grid, cont[0], t, cont[1], p, *cont[2:], host)
        acc.add_lines(*lines)
        acc.add_pseudo_continuum(*cont)
    got = acc.numpy()
    assert np.all(host[:, :-1] > 0) and np.array_equal(got, host)
    # the tensor IS the accumulator
    tt = acc.torch()
    assert tt.data_ptr() == acc.device_ptr() and tuple(tt.shape) == (L, nw) and tt.dtype == torch.float64
    assert np.array_equal(tt.cpu().numpy(), host)
    acc.add_pseudo_continuum(*isos[0][1])
    torch.cuda.synchronize()
    assert np.array_equal(tt.cpu().numpy(), acc.numpy()) and not np.array_equal(acc.numpy(), host)
    # begin starts over; the replaced object says so
    acc2 = eng.lbl_accumulator(wn_grid, t, p)
    assert not np.any(acc2.numpy())
    with pytest.raises(ValueError):
        acc.numpy()
    acc2.add_lines(*isos[0][0])
    one = np.zeros((L, nw))
    eng.add_line_set_monochromatic_absorption(wn_grid, isos[0][0][0], t, 296.0, p, *isos[0][0][2:], one)
    assert np.array_equal(acc2.numpy(), one)


def test_add_before_begin_raises():
    import archnemesis_dist_amd as pkg
    from archnemesis_dist_amd.engine import LblAccumulator
    e = pkg.AnsfmEngine(0)
    try:
        acc = LblAccumulator.__new__(LblAccumulator)         # an accumulator object whose context never saw `begin`
        acc._eng, acc.L, acc.nw = e, 1, 100
        e._lbl_accumulator = acc
        lines, cont = _gas(np.random.default_rng(1), np.linspace(2000.0, 2001.0, 100), 1)[0]
        with pytest.raises(ValueError, match="begin"):
            acc.add_lines(*lines)
        with pytest.raises(ValueError, match="begin"):
            acc.add_pseudo_continuum(*cont)
        with pytest.raises(ValueError, match="begin"):
            acc.numpy()
        with pytest.raises(ValueError, match="begin"):
            acc.device_ptr()
    finally:
        e.close()


def test_arguments(eng, golden):
    g = golden["regular"]
    nw = g["wn_grid"].shape[0]
    args = list(pc.engine_args(g))
    out = np.full(nw, 3.0)
    bad = list(args); bad[0] = g["wn_grid"][::-1].copy()
    with pytest.raises(ValueError):
        eng.add_pseudo_continuum_monochromatic_absorption(*bad, out)
    bad = list(args); c = g["centers"].copy(); c[[10, 11]] = c[[11, 10]]; bad[11] = c
    with pytest.raises(ValueError):
        eng.add_pseudo_continuum_monochromatic_absorption(*bad, out)
    bad = list(args); bad[1] = 7
    with pytest.raises(NotImplementedError):
        eng.add_pseudo_continuum_monochromatic_absorption(*bad, out)
    with pytest.raises(NotImplementedError):
        eng.add_pseudo_continuum_monochromatic_absorption(*args, out, n_neighbour_bins=9)
    none = list(args)
    none[10] = np.zeros((3, 0))
    for k in (11, 12, 13, 14):
        none[k] = np.zeros(0)
    eng.add_pseudo_continuum_monochromatic_absorption(*none, out)
    assert np.all(out == 3.0)                        # untouched by the refused calls and by N = 0
    # ... and the largest neighbour count that is built runs (onto zeros: opacities of 1e-25 vanish beside 3.0)
    most = np.zeros(nw)
    eng.add_pseudo_continuum_monochromatic_absorption(*args, most, n_neighbour_bins=8)
    assert np.count_nonzero(most) >= nw - 1 and np.all(most >= 0.0)
