"""The cases of tests/tile_edge_cases.py on the host: the oracle against the reference's own results (tests/golden/
tile_edges.npz, ILS), against a restatement of the same formulas in np.longdouble (weights, sums, cumulative sums,
interpolation), and the structure the cases are there for -- window and bin sizes on, below and above the kernels' chunk
sizes, positive total weights, every listed GEMM extent in use.

ILS_DEVIATION / KDIST_DEVIATION are what float64 arithmetic and the oracle's summation order cost against longdouble, per
case and output, as this test printed them; it measures them again and fails if one grows.  The GPU test's bound is
min(cap, 100 x deviation) with the cap the tolerance the kernel's existing test uses (ils_bounds, kdist_bound): measured
here on the host, never on the kernels.  A deviation of 0 gives the cap."""
import os

import numpy as np
import pytest

import tile_edge_cases as tc
from test_conv_oracle import close_nan

ILS_CASES = tc.ils_cases()
KDIST_CASES = tc.kdist_cases()
ORDINATES = {"g9": tc.G9, "g300": tc.g300()}

# (spectra, gradients): largest relative deviation of the oracle from longdouble (tc.ils_deviation)
ILS_DEVIATION = {
    "fil-128": (8.95e-16, 8.31e-14),
    "fil-129": (8.40e-16, 4.04e-12),
    "fil-130": (1.21e-15, 3.00e-14),
    "fil-y": (9.48e-16, 0.0),
    "fil-ngeom": (1.43e-15, 0.0),
    "filg-ngeom": (1.43e-15, 8.54e-14),
    "bracket-y": (1.08e-15, 0.0),
    "bracket-g": (1.08e-15, 4.90e-13),
    "intf-1": (1.59e-16, 0.0),
    "intfg-1": (2.54e-16, 1.09e-15),
    "intf-3": (1.22e-15, 0.0),
    "intfg-3": (1.22e-15, 3.95e-16),
    "shape0-g": (3.51e-16, 2.06e-14),
    "shape0-y": (3.51e-16, 0.0),
    "shape0-ngeom": (3.40e-16, 2.44e-13),
    "shape1-g": (3.55e-16, 6.44e-14),
    "shape1-y": (3.55e-16, 0.0),
    "shape1-ngeom": (1.02e-15, 1.08e-14),
    "shape2-g": (6.06e-16, 5.53e-14),
    "shape2-y": (6.06e-16, 0.0),
    "shape2-ngeom": (1.47e-15, 4.00e-14),
    "shape3-g": (3.17e-16, 3.36e-13),
    "shape3-y": (0.0, 0.0),
    "shape3-ngeom": (0.0, 0.0),
    "shape4-g": (0.0, 0.0),
    "shape4-y": (0.0, 0.0),
    "shape4-ngeom": (0.0, 0.0),
    "place-fil": (4.22e-17, 7.24e-14),
    "place-intf": (1.46e-16, 8.14e-17),
    "place-shape0": (1.17e-16, 2.35e-15),
    "place-shape1": (1.61e-16, 1.79e-14),
    "place-point": (0.0, 0.0),
    "repeat-fil": (1.08e-15, 1.95e-13),
    "repeat-intf": (1.87e-16, 9.37e-16),
    "repeat-shape1": (3.55e-16, 6.44e-14),
}
# (9 ordinates, 300 ordinates)
KDIST_DEVIATION = {
    "plain": (9.65e-16, 6.71e-15),
    "filter": (2.12e-14, 4.18e-14),
    "zero-weight": (0.0, 0.0),
    "ties": (0.0, 2.17e-15),
    "inf": (4.23e-16, 2.93e-15),
    "nan-pos": (4.23e-16, 2.93e-15),
    "nan-neg": (4.23e-16, 2.93e-15),
}


def ils_bounds(name):
    caps = tc.ILS_CAPS[tc.is_mean(ILS_CASES[name])]
    return tuple(min(cap, 100.0 * d) if d > 0.0 else cap for cap, d in zip(caps, ILS_DEVIATION[name]))


def kdist_bound(name, ordinates):
    d = KDIST_DEVIATION[name][list(ORDINATES).index(ordinates)]
    return min(tc.KDIST_CAP, 100.0 * d) if d > 0.0 else tc.KDIST_CAP


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "tile_edges.npz"))


def test_ils_structure():
    vw = tc.ils_grid()
    assert vw.size == 700 and np.all(np.diff(vw) > 0) and np.max(np.abs(vw - 2000.0 - 0.01 * np.arange(700))) <= 3e-3
    F = tc.ils_filters()
    assert tc.window_counts(vw, F) == tc.FIL_COUNTS == (3, 127, 257, 400, 4)
    assert tuple(F["nfil"]) == (2, 3, 7, 5, 2) and F["vfil"].shape == (7, 5)
    assert list(np.where(F["afil"][:7, 2] == 0.0)[0]) == [2, 4] and np.all(F["afil"][0] > 0.0)      # interior zeros; bracketing points weigh
    assert vw[0] < F["vfil"][0].min() and all(vw[-1] > F["vfil"][n - 1, j] for j, n in enumerate(F["nfil"]))
    assert tc.window_counts(vw, tc.placement_filters(vw)) == tc.PLACEMENT_COUNTS == (6, 6, 1, 0, 0, 3)
    P = tc.placement_filters(vw)
    assert P["vfil"][0, 0] < vw[0] and P["vfil"][1, 1] > vw[-1] and P["vfil"][0, 4] > vw[-1] and P["vfil"][0, 5] == vw[0]
    for ishape, n in tc.SHAPE_COUNTS.items():
        assert tc.shape_window_count(vw, ishape, tc.SHAPE_VCONV[0], tc.SHAPE_FWHM[ishape]) == n == {0: 128, 1: 129}[ishape]
    assert tc.shape_window_count(vw, 3, tc.SHAPE_VCONV[0], tc.SHAPE_FWHM[3]) == 129
    assert 3.6 * tc.SHAPE_FWHM[2] > 1.29 and 6 * tc.SHAPE_FWHM[4] > 1.29                            # more than one chunk
    vr = tc.ils_grid(repeat=True)
    assert vr[350] == vr[351] == vr[352] and np.all(np.diff(vr) >= 0) and tc.window_counts(vr, F) == tc.FIL_COUNTS
    ncol = lambda c: (0 if c["dydx"] is None else int(np.prod(c["dydx"].shape[1:]))) + (c["y"].shape[1] if c["y"].ndim == 2 else 1)
    assert [ncol(ILS_CASES["fil-%d" % n]) for n in (128, 129, 130)] == [128, 129, 130]
    assert ncol(ILS_CASES["filg-ngeom"]) == 42 * 3 + 3 > 128 and ILS_CASES["filg-ngeom"]["y"].shape[1] == 3
    # the windows at the ends of the grid, of one point and outside it
    c = ILS_CASES["place-shape0"]
    n = [tc.shape_window_count(vw, 0, v, c["fwhm"]) for v in c["vconv"]]
    assert n[0] > 1 and n[1] > 1 and n[3] == 0 and tc.shape_window_count(vw, 0, vw[200], ILS_CASES["place-point"]["fwhm"]) == 1
    e = tc.ils_exact_case()
    assert np.array_equal(e["y"], np.round(e["y"])) and np.array_equal(e["dydx"], np.round(e["dydx"])) and np.abs(e["dydx"]).max() == 8


def test_kdist_structure():
    c = KDIST_CASES["plain"]
    wave = c["wave"]
    assert tc.bin_counts(wave, c["lo"], c["hi"]) == tc.BIN_SIZES + (257,)
    first = [int(np.searchsorted(wave, a)) for a in c["lo"]]
    assert 0 in first and any(a + n == wave.size for a, n in zip(first, tc.BIN_SIZES))
    assert c["lo"][5] == c["lo"][10] and c["hi"][5] == c["hi"][10]                                   # two identical bins
    assert any(c["lo"][a] < c["lo"][b] < c["hi"][a] < c["hi"][b] for a in range(10) for b in range(10))   # bins overlap
    assert ORDINATES["g300"].size == 300 > 256 and ORDINATES["g300"][0] == 0.0 and ORDINATES["g300"][-1] == 1.0
    f = KDIST_CASES["filter"]
    lead = 0
    for b, n in enumerate(tc.bin_counts(wave, f["lo"], f["hi"])):
        w = tc.bin_weights(f, b)
        assert w.sum() > 0.0, b
        if n >= 255:                                        # both clamps reached: zero weight at both ends of the bin
            assert w[0] == 0.0 and w[-1] == 0.0 and f["fil"][2][3, b] - f["fil"][2][0, b] < f["hi"][b] - f["lo"][b]
        m = (wave >= f["lo"][b]) & (wave <= f["hi"][b])
        lead += int(w[np.argsort(f["kabs"][m], kind="stable")[0]] == 0.0)
    assert lead >= 3                                        # bins whose smallest k has zero weight: ordinate 0 tells the rules apart
    z = KDIST_CASES["zero-weight"]
    assert tc.bin_counts(wave, z["lo"], z["hi"]) == (50, 1) and not any(tc.bin_weights(z, b).any() for b in range(2))
    t = KDIST_CASES["ties"]
    assert np.unique(t["kabs"]).size == 6 and t["fil"] is None
    assert np.isposinf(KDIST_CASES["inf"]["kabs"]).sum() == 1
    for name, sign in (("nan-pos", False), ("nan-neg", True)):
        k = KDIST_CASES[name]["kabs"]
        assert np.isnan(k).sum() == 1 and bool(np.signbit(k[np.isnan(k)][0])) == sign
        m = (wave >= KDIST_CASES[name]["lo"][0]) & (wave <= KDIST_CASES[name]["hi"][0])
        assert np.isnan(k[m]).any()


def test_map_shapes_use_every_listed_value():
    cols = dict(W=0, NPRO=1, LIMAX=2, NPATH=3, NX=4)
    for name, values in tc.MAP_VALUES.items():
        assert set(values) <= {s[cols[name]] for s in tc.MAP_SHAPES}, name
    assert any(s[0] > 64 and s[1] > 64 and s[3] == 3 for s in tc.MAP_SHAPES)
    assert 8 <= len(tc.MAP_SHAPES) <= 12
    for i in tc.MAP_NEGATIVE_LAYINC:
        assert (tc.map_case(i)["LAYINC"] < 0).any()
    for i in tc.MAP_INCPAR_SUBSET:
        c = tc.map_case(i)
        assert list(c["INCPAR"]).index(c["NPAR"] - 1) > 0


@pytest.mark.parametrize("name", list(ILS_CASES) + ["exact"])
def test_ils_oracle_matches_the_reference(oracle, golden, name):
    c = tc.ils_exact_case() if name == "exact" else ILS_CASES[name]
    yo, go = tc.run_ils(oracle, c)
    if name == "exact":
        assert np.array_equal(yo, golden["exact/y"]) and np.array_equal(go, golden["exact/g"])
        return
    tight = c["y"].ndim == 2 or c["kind"] == "bracket"
    close_nan(yo, golden[name + "/y"], 1e-13)
    if go is not None and c["kind"] == "integrate":
        np.testing.assert_allclose(go, golden[name + "/g"], rtol=0, atol=1e-13 * np.abs(golden[name + "/g"]).max())
    elif go is not None:
        close_nan(go, golden[name + "/g"], 1e-13 if tight else 1e-12)
    else:
        assert name + "/g" not in golden.files


def test_ils_nan_and_zero_placement(golden):
    """outside the grid and between two grid points: 0/0 for the means, exactly 0 for the integrals"""
    assert list(np.isnan(golden["place-fil/y"])) == [False, False, False, True, True, False]
    assert np.array_equal(np.isnan(golden["place-fil/g"]).all(axis=1), np.isnan(golden["place-fil/y"]))
    for k in ("y", "g"):
        z = golden["place-intf/" + k]
        assert not z[2:5].any() and z[0].all() and z[1].all() and z[5].all()       # a single point integrates to 0 as well
    assert list(np.isnan(golden["place-shape0/y"])) == [False, False, False, True]
    assert np.isnan(golden["shape4-g/y"]).all() and np.isnan(golden["shape3-y/y"]).all()


@pytest.mark.parametrize("name", list(ILS_CASES))
def test_ils_deviation_from_longdouble(oracle, name):
    c = ILS_CASES[name]
    measured = tc.ils_deviation(tc.run_ils(oracle, c), tc.run_ils(tc.LD, c), tc.is_mean(c))
    print('    "%s": (%.2e, %.2e),' % ((name,) + measured))
    assert all(m <= r for m, r in zip(measured, ILS_DEVIATION[name])), (measured, ILS_DEVIATION[name])
    assert all(np.isfinite(b) and b <= cap for b, cap in zip(ils_bounds(name), tc.ILS_CAPS[tc.is_mean(c)]))


@pytest.mark.parametrize("name", list(KDIST_CASES))
def test_kdist_deviation_from_longdouble(oracle, name):
    c = KDIST_CASES[name]
    measured = tuple(tc.kdist_deviation(tc.run_kdist(oracle, c, g), tc.run_kdist(tc.LD, c, g)) for g in ORDINATES.values())
    print('    "%s": (%.2e, %.2e),' % ((name,) + measured))
    assert all(m <= r for m, r in zip(measured, KDIST_DEVIATION[name])), (measured, KDIST_DEVIATION[name])
    assert all(kdist_bound(name, o) <= tc.KDIST_CAP for o in ORDINATES)


def test_kdist_oracle_expectations(oracle):
    """what the GPU test asserts exactly, on the oracle: one point returns its k at every ordinate, ordinate 1 the largest k,
    ordinate 0 the smallest k unless the sorted order begins with zero weights -- then the k of the last of them"""
    for name in ("plain", "filter"):
        c = KDIST_CASES[name]
        r = tc.run_kdist(oracle, c, tc.G9)
        for b, n in enumerate(tc.bin_counts(c["wave"], c["lo"], c["hi"])):
            m = (c["wave"] >= c["lo"][b]) & (c["wave"] <= c["hi"][b])
            ks = np.sort(c["kabs"][m])
            assert np.array_equal(tc.run_kdist(oracle, tc.one_bin(c, b), tc.G9)[0], r[b])
            assert r[b, -1] == ks[-1]
            if n == 1:
                assert np.all(r[b] == ks[0])
            w = tc.bin_weights(c, b)[np.argsort(c["kabs"][m], kind="stable")]
            nz = int(np.argmax(w > 0.0))
            assert r[b, 0] == ks[max(nz - 1, 0)], (name, b)
    z = tc.run_kdist(oracle, KDIST_CASES["zero-weight"], tc.G9)
    assert np.isnan(z[0]).all() and np.all(z[1] == KDIST_CASES["zero-weight"]["kabs"][700])
    for name in ("nan-pos", "nan-neg"):                      # a NaN of either sign sorts last
        r = tc.run_kdist(oracle, KDIST_CASES[name], tc.G9)
        assert list(np.isnan(r[0])) == [False] * 7 + [True] * 2 and not np.isnan(r[1]).any()
    r = tc.run_kdist(oracle, KDIST_CASES["inf"], tc.G9)
    assert list(np.isposinf(r[0])) == [False] * 7 + [True] * 2 and np.isfinite(r[1]).all()


@pytest.mark.parametrize("i", range(len(tc.MAP_SHAPES)))
def test_integer_maps_are_exact(oracle, i):
    c = tc.map_case(i)
    pro = oracle.map2pro(c["dSPECIN"], *tc.map2pro_args(c), INCPAR=c["INCPAR"])
    xvec = oracle.map2xvec(pro, *tc.map2xvec_args(c))
    P, _, X, _ = tc.map_longdouble(c, pro)
    assert np.array_equal(pro, P.astype(float)) and np.array_equal(xvec, X.astype(float))
    assert np.abs(X).max() < 2.0 ** 53 and pro.any() and xvec.any()


def test_real_map_bound_holds_for_the_oracle(oracle):
    c = tc.map_case(len(tc.MAP_SHAPES) - 1, real=True)
    pro = oracle.map2pro(c["dSPECIN"], *tc.map2pro_args(c), INCPAR=c["INCPAR"])
    xvec = oracle.map2xvec(pro, *tc.map2xvec_args(c))
    P, Pabs, X, Xabs = tc.map_longdouble(c, pro)
    u = 2.0 ** -53
    assert np.all(np.abs(pro - P) <= 2 * c["LIMAX"] * u * Pabs)
    assert np.all(np.abs(xvec - X) <= 2 * c["NPAR"] * c["NPRO"] * u * Xabs)
