"""The NumPy restatement of the surface BRDF and the BRDF matrix (tests/brdf_cases.py) against the reference's results in
tests/golden/brdf.npz (tools/golden/gen_golden_brdf.py): within 1e-13 of the row (matrix: plane) maximum, which is what makes
it the contract the kernels are written to; the shapes; the cases the golden holds are the cases of brdf_cases.py; and the
stored one-ulp figures keep every GPU bound (16 x) at or below the project's parity bar of 1e-6.  No GPU."""
import os

import numpy as np
import pytest

import brdf_cases as bc

CASES = bc.POINT_CASES + bc.MATRIX_CASES


@pytest.fixture(scope="module")
def golden(golden_dir):
    return bc.load_golden(os.path.join(golden_dir, "brdf.npz"))


def test_golden_holds_the_cases(golden):
    cases = bc.golden_cases()
    assert tuple(golden) == tuple(cases) == CASES
    for name, d in cases.items():
        g = golden[name]
        assert g["kind"] == d["kind"]
        for k in bc.INPUTS[d["kind"]]:
            assert np.array_equal(g[k], d[k]), (name, k)


@pytest.mark.parametrize("name", CASES)
def test_restatement(golden, name):
    g = golden[name]
    got = bc.evaluate_np(g)
    W = g["params"].shape[1]
    if g["kind"] == "points":
        assert got.shape == g["ref"].shape == (W, bc.NTHETA)
    else:
        nmu = g["MU"].shape[0]
        assert got.shape == g["ref"].shape == (W, nmu, nmu, int(g["NF"]) + 1)
    assert bc.deviation(got, g["ref"]) <= 1e-13


def test_gpu_bounds_are_within_the_parity_bar(golden):
    for name, g in golden.items():
        assert 0.0 <= 16.0 * float(g["ulp"]) <= 1e-6, name


def test_the_cases_reach_the_branches(golden):
    """what the array-level cases are there for, read off the inputs: both orders of (i, e) and equality, zero and dark
    angles, the azimuths on both sides of the fold, cg below 0 before the clamp, exact opposition only where hs, hc >= 0.5"""
    g = golden["hapke-opposition"]
    i, e, a = g["sol"], g["emi"], g["azi"]
    assert np.any(i < e) and np.any(i > e) and np.any((i == e) & (i > 0)) and np.any(e == 0) and np.any(i == 0)
    assert np.any(e == 90.) and np.any(i == 95.) and {0., 180., 360., 200., 359.9} <= set(a.tolist())
    assert np.any((i == 60.) & (e == 60.) & (a == 0.))
    lit = (i < 90) & (e < 90)
    assert np.all(g["ref"][:, ~lit] == 0) and np.all(g["ref"][:, lit] > 0)
    assert g["params"][6, 1] == 0.0 and g["params"][0, 2] == 0.999
    opposition = lambda d: np.any((d["sol"] == d["emi"]) & ((d["azi"] == 180.) | (d["sol"] == 0)))
    assert opposition(g) and min(g["params"][3].min(), g["params"][5].min()) >= 0.5
    n = golden["hapke-narrow"]
    assert not opposition(n) and max(n["params"][3].max(), n["params"][5].max()) < 0.1
    o = golden["oren-nayar"]
    c = np.cos(np.radians(o["azi"]))
    assert np.any(c > 0.1) and np.any(c < -0.1) and np.any(o["params"][1] == 0.0)
    assert bc.fold_azimuth(360.00000000000006) == 180.00000000000006 and bc.matrix_tables(np.ones(1), 100, 0)[1][-1] > 360.0


def test_lambert_and_oren_nayar_matrices(golden):
    g = golden["m-lambert"]
    assert np.array_equal(g["ref"][..., 0], np.broadcast_to((g["params"][0] / np.pi)[:, None, None], g["ref"].shape[:3]))
    assert not np.any(g["ref"][..., 1:]) and not np.any(golden["m-oren-nayar"]["ref"])
