"""k_ils_conv, k_kdist_gather / k_kdist_quantiles and k_gemm_f64 on the GPU at their tile, chunk and clamp edges (tests/
tile_edge_cases.py) against oracle/oracle.py: filter windows of 3, 127, 257, 400 and 4 points and 128, 129 and 130 columns
(second chunk, second column block, the trapezoid weights across a chunk seam, the bracketing window), windows at both ends
of the grid, of one point, of none and outside the grid, repeated wavenumbers; bins of 1 to 1000 points around the scan's
256 chunks, both filter clamps, zero weights, tied k, +inf and a NaN of either sign, 300 g-ordinates; GEMM extents on, below
and above 64 and 16 in M, N and K with 1 and 3 paths.

Bounds per case and output: min(cap, 100 x deviation) with the deviation of the oracle from np.longdouble measured on the host
(tests/test_tile_edges_host.py: ILS_DEVIATION, KDIST_DEVIATION) and the cap the tolerance of the kernel's existing test.  The
integer-valued cases are exact in float64 and must match bit for bit.

Measured on MI355X: see the table there."""
import numpy as np
import pytest

import tile_edge_cases as tc
from test_tile_edges_host import ILS_CASES, KDIST_CASES, ORDINATES, ils_bounds, kdist_bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from archnemesis_dist_amd.engine import AnsfmEngine
    eng = AnsfmEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def kdist_reference(oracle):
    """the oracle's k-distributions of every case, computed once and shared"""
    ref = {(name, o): tc.run_kdist(oracle, c, g) for name, c in KDIST_CASES.items() for o, g in ORDINATES.items()}
    for r in ref.values():
        r.flags.writeable = False
    return ref


# ---- ILS ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ILS_CASES))
def test_ils_cases(engine, oracle, name):
    c = ILS_CASES[name]
    want = tc.run_ils(oracle, c)
    got = tc.run_ils(engine, c)
    dev = tc.ils_deviation(got, want, tc.is_mean(c))
    bounds = ils_bounds(name)
    print("%s: spectra %.2e  gradients %.2e  (bounds %.1e %.1e)" % ((name,) + dev + bounds))
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if b is not None:
            assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))      # NaN parity, as close_nan asks
    assert all(d <= b for d, b in zip(dev, bounds)), (dev, bounds)


def test_ils_outside_the_grid(engine):
    """no point inside the filter: 0/0 for the means, exactly 0 for the integrals -- one point integrates to 0 as well"""
    yo, go = tc.run_ils(engine, ILS_CASES["place-fil"])
    assert list(np.isnan(yo)) == [False, False, False, True, True, False]
    assert np.array_equal(np.isnan(go).all(axis=1), np.isnan(yo)) and np.array_equal(np.isnan(go).any(axis=1), np.isnan(yo))
    yo, go = tc.run_ils(engine, ILS_CASES["place-intf"])
    assert not yo[2:5].any() and not go[2:5].any() and yo[[0, 1, 5]].all() and go[[0, 1, 5]].all()


def test_ils_integer_case_is_bit_identical(engine, oracle):
    c = tc.ils_exact_case()
    want = tc.run_ils(oracle, c)
    got = tc.run_ils(engine, c)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert want[1].shape == (5, 129) and np.isfinite(want[1]).all()


# ---- k-distribution ------------------------------------------------------------------------------------------------------
def _check_kdist(got, want, name, o, what):
    dev = tc.kdist_deviation(got, want)
    bound = kdist_bound(name, o)
    print("%s %s %s: %.2e (bound %.1e)" % (name, o, what, dev, bound))
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (name, o, what, got, want)
    assert dev <= bound, (name, o, what, dev, bound)


@pytest.mark.parametrize("o", list(ORDINATES))
@pytest.mark.parametrize("name", ["plain", "filter"])
def test_kdist_bin_sizes(engine, kdist_reference, name, o):
    """every bin alone and all in one call; the exact expectations at the ordinates 0 and 1 and for a single point"""
    c = KDIST_CASES[name]
    want = kdist_reference[name, o]
    joint = tc.run_kdist(engine, c, ORDINATES[o])
    _check_kdist(joint, want, name, o, "all bins")
    sizes = tc.bin_counts(c["wave"], c["lo"], c["hi"])
    for b, n in enumerate(sizes):
        alone = tc.run_kdist(engine, tc.one_bin(c, b), ORDINATES[o])
        _check_kdist(alone, want[b:b + 1], name, o, "bin %d of %d points" % (b, n))
        assert np.array_equal(alone[0], joint[b]), (b, n)
        m = (c["wave"] >= c["lo"][b]) & (c["wave"] <= c["hi"][b])
        ks = np.sort(c["kabs"][m])
        assert joint[b, -1] == ks[-1], (b, n)                        # ordinate 1: the largest k
        if n == 1:
            assert np.all(joint[b] == ks[0])
        if name == "plain":
            assert joint[b, 0] == ks[0], (b, n)                      # ordinate 0 without leading zero weights: the smallest k
    assert np.array_equal(joint[5], joint[10])                       # the two identical bins
    # ordinate 0 with leading zero weights: the k of the last zero-weight point, as np.interp picks it
    assert np.array_equal(joint[:, 0], want[:, 0]), (joint[:, 0], want[:, 0])


@pytest.mark.parametrize("o", list(ORDINATES))
@pytest.mark.parametrize("name", ["zero-weight", "ties", "inf", "nan-pos", "nan-neg"])
def test_kdist_values(engine, kdist_reference, name, o):
    got = tc.run_kdist(engine, KDIST_CASES[name], ORDINATES[o])
    _check_kdist(got, kdist_reference[name, o], name, o, "all bins")
    if name == "zero-weight":
        assert np.isnan(got[0]).all() and np.all(got[1] == KDIST_CASES[name]["kabs"][700])
    if name == "ties":                                               # ordinates 0 and 1 land on levels
        assert np.array_equal(got[:, [0, -1]], kdist_reference[name, o][:, [0, -1]])


# ---- gradient maps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(tc.MAP_SHAPES)))
def test_integer_maps_are_bit_identical(engine, oracle, i):
    c = tc.map_case(i)
    pro = oracle.map2pro(c["dSPECIN"], *tc.map2pro_args(c), INCPAR=c["INCPAR"])
    xvec = oracle.map2xvec(pro, *tc.map2xvec_args(c))
    got = engine.map2pro(c["dSPECIN"], *tc.map2pro_args(c), INCPAR=c["INCPAR"])
    assert got.shape == pro.shape and np.array_equal(got, pro)
    assert np.array_equal(engine.map2xvec(got, *tc.map2xvec_args(c)), xvec)                  # continues from the device copy
    assert np.array_equal(engine.map2xvec(pro.copy(), *tc.map2xvec_args(c)), xvec)           # uploaded
    assert engine.map2pro(c["dSPECIN"], *tc.map2pro_args(c), INCPAR=c["INCPAR"], to_host=False) is None
    assert np.array_equal(engine.map2xvec(None, *tc.map2xvec_args(c)), xvec)                 # device-chained, nothing copied back


def test_real_maps_within_the_product_bound(engine, oracle):
    """the largest shape with real entries: |C - C_ld| <= 2 K 2^-53 (|A| . |B|) element by element, K the depth of the product"""
    c = tc.map_case(len(tc.MAP_SHAPES) - 1, real=True)
    u = 2.0 ** -53
    K1, K2 = c["LIMAX"], c["NPAR"] * c["NPRO"]
    got = engine.map2pro(c["dSPECIN"], *tc.map2pro_args(c), INCPAR=c["INCPAR"])
    P, Pabs, X, Xabs = tc.map_longdouble(c, got)
    assert np.all(np.abs(got - P) <= 2 * K1 * u * Pabs)
    print("map2pro: largest |C - C_ld| / (2 K u |A|.|B|) = %.3f" % float(np.max(np.abs(got - P)[Pabs > 0] / (2 * K1 * u * Pabs[Pabs > 0]))))
    # map2xvec of the very array map2pro returned, from its device copy and uploaded again: the same input, the same bound
    for xin in (got, got.copy()):
        x = engine.map2xvec(xin, *tc.map2xvec_args(c))
        assert np.all(np.abs(x - X) <= 2 * K2 * u * Xabs)
        print("map2xvec: largest |C - C_ld| / (2 K u |A|.|B|) = %.3f" % float(np.max(np.abs(x - X) / (2 * K2 * u * Xabs))))
