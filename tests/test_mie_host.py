"""makephase_np (tests/mie_cases.py), the NumPy restatement that is the written-down contract of the Mie kernels, against the
reference's results in tests/golden/mie.npz.  CPU only, no reference needed.  The deviation with the kernels' order of the
sum over radii (chunks of 64, a tree inside a chunk) isolates what that order costs; 100 times the largest of these
deviations over the cases is the bound of the GPU test (tests/test_mie_gpu.py), see DESIGN.md 4.5e.  The edge cases
(tests/golden/mie_edges.npz, tests/test_mie_edges_gpu.py) have a bound each, which also counts how strongly the case amplifies
one ulp in sin, cos, exp, log and pow: EDGE_DEVIATION."""
import os

import numpy as np
import pytest

import mie_cases as mc

CASES = tuple(mc.golden_cases())
# the largest deviations over the cases with the kernels' summation order, as this test printed them where the golden was
# made (cross-sections, phase function relative to its maximum, phase function point by point): x 100 = the GPU test's bounds
CHUNK_ORDER_DEVIATION = (1.92e-15, 1.68e-15, 4.18e-15)

EDGE_CASES = tuple(mc.edge_cases())
# per edge case the larger of its chunk-order deviation and its one-ulp sensitivity (mc.one_ulp_sensitivity: how strongly
# the case amplifies a last-place difference in sin, cos, exp, log and pow, the only thing the device may round otherwise),
# as tools/golden/gen_golden_mie.py printed them where tests/golden/mie_edges.npz was made, rounded up: x 100, capped at
# 1e-6, = the bounds of tests/test_mie_edges_gpu.py.  This test measures both again and holds the record to be no smaller.
EDGE_DEVIATION = {
    "perwave-m": (1.88e-15, 1.62e-14, 1.62e-14),
    "nmx150": (1.23e-15, 2.09e-16, 8.53e-16),
    "x2000-single": (6.93e-15, 1.23e-15, 5.60e-14),
    "absorbing": (5.33e-16, 2.40e-15, 2.40e-15),
    "small-x": (7.81e-12, 3.38e-11, 3.38e-11),
    "fail-behind-cut": (4.09e-16, 1.11e-15, 4.60e-15),
    "closed-2": (1.72e-14, 2.29e-13, 2.29e-13),
    "theta-0": (5.13e-16, 6.14e-15, 6.14e-15),
    "theta-90": (5.13e-16, 5.14e-16, 5.14e-16),
    "theta-33": (5.13e-16, 6.14e-15, 6.18e-15),
    "theta-33-90": (5.13e-16, 6.14e-15, 6.18e-15),
    "waves-130": (3.20e-14, 3.64e-13, 3.64e-13),
    "ws-halved": (2.23e-15, 2.12e-15, 5.98e-15),
    "open-64": (5.63e-16, 8.23e-16, 8.23e-16),
    "open-65": (4.50e-16, 4.12e-16, 4.41e-16),
    "open-128": (1.35e-15, 6.86e-16, 1.04e-15),
    "open-129": (7.88e-16, 6.86e-16, 8.32e-16),
}
# the restatement's pointwise deviation from the reference where 1e-14 does not hold it, as the generator printed it: the
# single sphere at x = 2011, whose phase function falls below 1e-7 of its forward peak
EDGE_POINTWISE = {"x2000-single": 5.6e-14}
# 64 wavelengths x 300 radii at x up to 829 take the restatement a quarter of a minute per evaluation: the sensitivity
# (two more evaluations) is measured, and asserted against the record, by the generator only
SENSITIVITY_NOT_RERUN = ("ws-halved",)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return mc.load_golden(os.path.join(golden_dir, "mie.npz"))


def test_golden_holds_the_cases(golden):
    cases = mc.golden_cases()
    assert set(golden) == set(cases)
    for name, d in cases.items():
        for k in mc.INPUTS:
            assert np.array_equal(golden[name][k], d[k]), (name, k)
        assert golden[name]["phas"].shape == (d["wavel"].shape[0], mc.nphas_of(d["theta"]))
    assert golden["gamma-open-no90"]["phas"].shape[1] == 6 and golden["lognormal-open-90"]["phas"].shape[1] == 7
    assert list(golden["lognormal-open-90"]["n_radii"]) == [177, 199, 234]
    assert list(golden["gamma-open-no90"]["n_radii"]) == [205, 226]
    for name, n in mc.EXPECTED_RADII.items():
        assert np.all(golden[name]["n_radii"] == n), name


@pytest.mark.parametrize("chunk_order", [False, True], ids=["reference order", "chunk order"])
@pytest.mark.parametrize("name", CASES)
def test_restatement_against_the_reference(golden, name, chunk_order):
    g = golden[name]
    xs, xe, thetax, ph, counts = mc.makephase_np(g["wavel"], g["iscat"], g["dsize"], g["rs"], g["refindx"], g["theta"],
                                                 chunk_order=chunk_order, return_counts=True)
    dev = mc.deviations((xs, xe, ph), g)
    print("%s (%s): cross-sections %.2e  phase / max %.2e  phase pointwise %.2e" %
          (name, "chunk order" if chunk_order else "reference order", *dev))
    assert np.array_equal(counts, g["n_radii"]) and np.array_equal(thetax, g["thetax"])
    # the restatement follows the reference operation by operation: what is left are the complex divisions (Python's
    # form in places there, NumPy's here) and the order of the sum over at most 453 radii, a few ulp each
    assert max(dev) <= 1e-14, dev


@pytest.fixture(scope="module")
def edges(golden_dir):
    return mc.load_golden(os.path.join(golden_dir, "mie_edges.npz"))


def test_edges_golden_holds_the_cases(edges):
    cases = mc.edge_cases()
    assert set(edges) == set(cases) == set(EDGE_DEVIATION) == set(mc.EDGE_EXPECTED_RADII) and not set(cases) & set(CASES)
    for name, d in cases.items():
        for k in mc.INPUTS:
            assert np.array_equal(edges[name][k], d[k]), (name, k)
        assert edges[name]["phas"].shape == (d["wavel"].shape[0], mc.nphas_of(d["theta"]))
        assert np.all(edges[name]["n_radii"] == mc.EDGE_EXPECTED_RADII[name]), name
        assert (mc.radius_count(d["rs"]) is None) == (name in mc.EDGE_OPEN_CASES)
    assert [edges[n]["phas"].shape[1] for n in ("theta-0", "theta-90", "theta-33", "theta-33-90")] == [2, 1, 66, 65]
    x = lambda n: 2.0 * np.pi * (cases[n]["rs"][0] + np.arange(edges[n]["n_radii"][0]) * cases[n]["rs"][2]) / cases[n]["wavel"][0]
    assert 3e-3 <= x("small-x").min() and x("small-x").max() <= 3e-2
    assert 1.1 * 1.5 * x("nmx150").min() < 150 < 151 < 1.1 * 1.5 * x("nmx150").max()
    # the default block of 512 radii would take more than the 1 GiB the workspace may have, half of it does not
    d = cases["ws-halved"]
    rows = 2.0 * np.pi * (d["rs"][0] + 299 * d["rs"][2]) * np.max(np.hypot(*d["refindx"].T) / d["wavel"])
    assert rows * 6 * 64 * 256 * 8 < 2 ** 30 < rows * 6 * 64 * 512 * 8


@pytest.mark.parametrize("name", EDGE_CASES)
def test_edge_restatement_against_the_reference(edges, name):
    """Both orders of the sum from one evaluation of the series (the memo): `ws-halved` takes a quarter of a minute."""
    g = edges[name]
    args = (g["wavel"], g["iscat"], g["dsize"], g["rs"], g["refindx"], g["theta"])
    memo, dev = {}, {}
    for chunk_order in (False, True):
        xs, xe, thetax, ph, counts = mc.makephase_np(*args, chunk_order=chunk_order, return_counts=True, memo=memo)
        dev[chunk_order] = mc.deviations((xs, xe, ph), g)
        print("%s (%s): cross-sections %.2e  phase / max %.2e  phase pointwise %.2e" %
              (name, "chunk order" if chunk_order else "reference order", *dev[chunk_order]))
        assert np.array_equal(counts, g["n_radii"]) and np.array_equal(thetax, g["thetax"])
        assert max(dev[chunk_order][:2]) <= 1e-14, dev[chunk_order]
        # 10 x what the restatement showed where the golden was made: headroom for a NumPy whose complex division differs
        assert dev[chunk_order][2] <= 10.0 * EDGE_POINTWISE.get(name, 1e-15), dev[chunk_order]
    measured = dev[True]
    if name not in SENSITIVITY_NOT_RERUN:
        sens = mc.one_ulp_sensitivity(g)
        print("%s: one ulp in sin, cos, exp, log, pow moves %.2e %.2e %.2e" % ((name,) + sens))
        measured = tuple(max(a, b) for a, b in zip(measured, sens))
    assert all(m <= r for m, r in zip(measured, EDGE_DEVIATION[name])), (measured, EDGE_DEVIATION[name])
    assert all(100.0 * r <= 1e-6 for r in EDGE_DEVIATION[name])       # the GPU bound stays under the parity bar's cap


@pytest.mark.parametrize("name", ["perwave-m", "waves-130"])
def test_edges_tell_a_shared_index_apart(edges, name):
    """what these two cases are for: with the first wavelength's index at every wavelength the results are far off"""
    g = edges[name]
    xs, xe, _, ph = mc.makephase_np(g["wavel"], g["iscat"], g["dsize"], g["rs"], np.tile(g["refindx"][0], (g["wavel"].shape[0], 1)),
                                    g["theta"])
    assert min(mc.deviations((xs, xe, ph), g)) > 1e-3


def test_one_ulp_shift_moves_every_elementary_function():
    x = np.array([0.3, 2.0])
    for direction in (1.0, -1.0):
        fn = mc.shifted_funcs(direction)
        for name in ("cos", "exp", "log"):
            assert np.array_equal(getattr(fn, name)(x), np.nextafter(getattr(np, name)(x), direction * np.inf)), name
        assert np.array_equal(fn.pow(x, 1.5), np.nextafter(x ** 1.5, direction * np.inf))
        assert np.array_equal(fn.sin(x), np.nextafter(np.sin(x), -direction * np.inf))
    d = mc.edge_cases()["small-x"]
    cross, norm, point = mc.one_ulp_sensitivity(d)
    # 2e-14 / x^2: at the case's smallest x = 3.0e-3 that is 2e-9, the distribution's weight lies at larger x
    assert 1e-13 < cross < 3e-9 and 1e-13 < point < 3e-9


def test_chunk_order_is_a_different_order(golden):
    g = golden["closed-65"]
    a = mc.makephase_np(g["wavel"], g["iscat"], g["dsize"], g["rs"], g["refindx"], g["theta"])
    b = mc.makephase_np(g["wavel"], g["iscat"], g["dsize"], g["rs"], g["refindx"], g["theta"], chunk_order=True)
    assert not np.array_equal(a[3], b[3]) and np.allclose(a[3], b[3], rtol=1e-13, atol=0)


def test_failures_are_raised():
    d = mc.golden_cases()["lognormal-open-90"]
    with pytest.raises(ValueError):
        mc.makephase_np(d["wavel"], 2, d["dsize"], d["rs"], d["refindx"], [0.0, 95.0])
    with pytest.raises(mc.MieFailure, match="did not terminate"):
        mc.makephase_np(d["wavel"], 2, d["dsize"], d["rs"], d["refindx"], d["theta"], cap=128)
    # x = 201, m = 1.05: the series needs more than nmx2 = int(1.05 x) terms (the reference fails on this input too)
    with pytest.raises(mc.MieFailure, match="radius 16 um"):
        mc.makephase_np([0.5], 4, [16.0, 0, 0], [16.0, 16.0, 16.0], [[1.05, 0.0]], [0.0, 90.0])
