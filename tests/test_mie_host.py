"""makephase_np (tests/mie_cases.py), the NumPy restatement that is the written-down contract of the Mie kernels, against the
reference's results in tests/golden/mie.npz.  CPU only, no reference needed.  The deviation with the kernels' order of the
sum over radii (chunks of 64, a tree inside a chunk) isolates what that order costs; 100 times the largest of these
deviations over the cases is the bound of the GPU test (tests/test_mie_gpu.py), see DESIGN.md 4.5e."""
import os

import numpy as np
import pytest

import mie_cases as mc

CASES = tuple(mc.golden_cases())
# the largest deviations over the cases with the kernels' summation order, as this test printed them where the golden was
# made (cross-sections, phase function relative to its maximum, phase function point by point): x 100 = the GPU test's bounds
CHUNK_ORDER_DEVIATION = (1.92e-15, 1.68e-15, 4.18e-15)


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
