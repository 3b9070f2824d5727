"""A model in NumPy of the test that lets the forward merge walk a merge row by row without its head list
(merge_rowmajor_test in csrc/ansfm_merge64.hip.h).

A lane's G x G sums rows[i] + cols[j] are popped in ascending order of their list keys: the double with its low 11 bits replaced
by (col << 5) | row or, in a lane whose rows are b ("swapped", MergeOrient), by (row << 6) | col.  The kernel's test compares
the last key of every row with the next entry of the (sorted) head list, K(i, G-1) < R[i+1] for i + 1 < G; what it has to decide
is whether the ascending-key order is the row-major order.  Both are restated here and must agree in both directions -- the
test is exact, not merely sufficient -- for every G of every instantiated list length, for random operands at magnitude
ratios 1 ... 1e-12, and for constructed ties in both orientations: r_i + c_{G-1} and r_{i+1} + c_0 equal in their top 53 bits
(the low bits decide, differently in the two packings), flat operands, equal neighbouring rows.  Heads that are not
ascending fail it.  No GPU: this pins the argument, tests/test_merge_rowmajor.py pins the kernel."""
import numpy as np
import pytest

LIST_LENGTHS = [8, 10, 16, 20, 32]
ALL_G = list(range(2, 33))                       # every G <= NR of every list length (the division-free walk needs G >= 2)
RATIOS = [10.0 ** -e for e in range(13)]         # 1 ... 1e-12
MASK = np.uint64(0x7FF)


def list_len(G):
    return next(v for v in LIST_LENGTHS if v >= G)


def swap_choice(a, b):
    """The kernel's orientation: rows = the operand with the larger top ordinate; b only where a is non-decreasing."""
    return bool(b[-1] > a[-1] and np.all(np.diff(a) >= 0))


def lane_keys(rows, cols, swapped):
    """K[i, j]: the list key of element (row i, column j) as this lane packs it, as the 64-bit pattern (the sums are >= +0, so
    the patterns compare like the doubles)."""
    G = len(rows)
    s = np.add.outer(np.asarray(rows, np.float64), np.asarray(cols, np.float64))
    i, j = np.meshgrid(np.arange(G, dtype=np.uint64), np.arange(G, dtype=np.uint64), indexing="ij")
    low = (i << np.uint64(6)) | j if swapped else (j << np.uint64(5)) | i
    return (s.view(np.uint64) & ~MASK) | low


def kernel_test(K):
    """merge_rowmajor_test: the heads as merge_init leaves them (sorted when they were not ascending), then
    K(i, G-1) < R[i+1] for every i + 1 < G."""
    R = np.sort(K[:, 0])
    return bool(np.all(K[:-1, -1] < R[1:]))


def pops_row_major(K):
    """The list merge pops keys in ascending order (they are distinct: the low bits differ): is that row by row?"""
    flat = K.ravel()
    return bool(np.all(flat[:-1] < flat[1:]))


def lane_passes(a, b):
    """Orientation and test of one lane for the operands a (the merged spectrum so far) and b (the next gas)."""
    sw = swap_choice(a, b)
    rows, cols = (b, a) if sw else (a, b)
    return kernel_test(lane_keys(rows, cols, sw))


def random_operand(rng, G, decades=2.0):
    return np.sort(10.0 ** rng.uniform(-decades, decades, G))


def tie_operands(G, nudge=0):
    """Rows with gap 8 and columns spanning exactly 8: r_i + c_{G-1} = r_{i+1} + c_0 in every bit (nudge = 0) or up to `nudge`
    units of the last place, well inside the 11 bits a key drops.  The low bits decide: (col << 5) | row puts K(i, G-1) above
    K(i+1, 0), (row << 6) | col below."""
    r = 1024.0 + 8.0 * np.arange(G)
    c = np.linspace(0.0, 8.0, G)
    c[-1] = 8.0 + nudge * 2.0 ** -42               # ulp of the sums (1024 <= sum < 2048) is 2^-42
    return r, c


@pytest.mark.parametrize("G", ALL_G)
def test_random_operands(G):
    """Both directions at every magnitude ratio, either operand the large one; across the ratios both outcomes occur."""
    rng = np.random.default_rng(500 + G)
    seen = set()
    for ratio in RATIOS:
        for _ in range(20):
            big, small = random_operand(rng, G), ratio * random_operand(rng, G)
            for a, b in ((big, small), (small, big)):
                sw = swap_choice(a, b)
                rows, cols = (b, a) if sw else (a, b)
                K = lane_keys(rows, cols, sw)
                assert kernel_test(K) == pops_row_major(K), (G, ratio, sw)
                seen.add((sw, kernel_test(K)))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}, seen


@pytest.mark.parametrize("nudge", [0, 1, -1, 3, -3, 500, -500])
@pytest.mark.parametrize("G", ALL_G)
def test_ties_across_the_row_boundary(G, nudge):
    r, c = tie_operands(G, nudge)
    for swapped in (False, True):
        a, b = (c, r) if swapped else (r, c)
        assert swap_choice(a, b) == swapped
        K = lane_keys(r, c, swapped)
        assert kernel_test(K) == pops_row_major(K), (G, nudge, swapped)
        if nudge >= 0:
            assert (K[:-1, -1] & ~MASK == K[1:, 0] & ~MASK).all()    # the top 53 bits do tie: the packing decides
            assert kernel_test(K) == swapped, (G, nudge, swapped)
        else:                                                        # one unit below borrows through the dropped bits: no tie
            assert (K[:-1, -1] & ~MASK < K[1:, 0] & ~MASK).all() and kernel_test(K)


@pytest.mark.parametrize("G", ALL_G)
def test_flat_operands_and_equal_rows(G):
    rng = np.random.default_rng(900 + G)
    flat1, flat2 = np.full(G, 3.0), np.full(G, 3.5)
    for a, b in ((flat2, flat1), (flat1, flat2), (flat1, flat1)):       # unswapped, swapped, unswapped (equal tops)
        sw = swap_choice(a, b)
        rows, cols = (b, a) if sw else (a, b)
        K = lane_keys(rows, cols, sw)
        assert kernel_test(K) == pops_row_major(K) == sw, (G, sw)        # every key ties: the packing alone decides
    for ratio in (1.0, 1e-6, 1e-14, 0.0):
        rows = random_operand(rng, G) + 10.0
        rows[G // 2] = rows[G // 2 - 1]                                 # two equal neighbouring rows
        cols = ratio * random_operand(rng, G) if ratio else np.zeros(G)
        for sw in (False, True):
            K = lane_keys(rows, cols, sw)
            assert kernel_test(K) == pops_row_major(K), (G, ratio, sw)
    # equal rows and columns too small to show in a key: row-major in the swapped packing only
    rows = np.repeat(np.arange(1.0, G // 2 + 2), 2)[:G] * 1024.0
    cols = np.arange(G) * 2.0 ** -45
    assert pops_row_major(lane_keys(rows, cols, True)) and kernel_test(lane_keys(rows, cols, True))
    assert not pops_row_major(lane_keys(rows, cols, False)) and not kernel_test(lane_keys(rows, cols, False))


@pytest.mark.parametrize("G", ALL_G)
def test_unsorted_heads_fail(G):
    """A merged spectrum is ascending only up to rounding: with a neighbour pair of rows out of order beyond a key's
    precision the heads are not ascending, merge_init sorts them, and the test on the sorted heads must still fail --
    however small the columns are."""
    rng = np.random.default_rng(1300 + G)
    for ratio in (1e-3, 1e-9, 1e-15, 0.0):
        for _ in range(10):
            rows = random_operand(rng, G) + 1.0
            i = int(rng.integers(0, G - 1))
            rows[i], rows[i + 1] = rows[i + 1] * (1.0 + 1e-9), rows[i]      # out of order, far above 2^-41 relative
            cols = ratio * random_operand(rng, G) if ratio else np.zeros(G)
            K = lane_keys(rows, cols, False)                                # such a lane is never swapped
            assert K[i, 0] > K[i + 1, 0]                                    # the heads are not ascending
            assert not pops_row_major(K)
            assert not kernel_test(K), (G, ratio, i)


def test_every_list_length_has_its_g():
    assert sorted({list_len(G) for G in ALL_G}) == LIST_LENGTHS
    # the columns the walk takes without a guard exist at every G of the list length (merge_rowmajor_sure_cols)
    sure = {8: 2, 10: 9, 16: 11, 20: 17, 32: 21}
    for G in ALL_G:
        assert sure[list_len(G)] <= G
