"""A model in plain Python / NumPy of the partial form of the forward merge's row walk (merge_rowmajor_test, merge_suffix_row and
k_ck_overlap in csrc/): a merge whose rows i0 .. G-1 sort row by row above everything in the rows below runs the register list
for the G * i0 elements of those rows only and walks the rest.

Restated here: the list keys of a lane in both packings (tests/test_merge_rowmajor_model.py), the register list with its
insertion network and sentinels (merge_step), and the rule for i0.  With R the sorted heads and M(i) the largest last key
K(i', G-1) of the rows i' <= i, boundary i passes when M(i) < R[i+1]; a lane's i0 is 0 when every boundary passes and else the
last failing boundary + 2 (so 1 never occurs: boundaries 0 .. G-2 all passing is the whole walk), the wave's the largest of its
lanes'.  (The kernels of the lists shorter than 16 entries do not take a suffix: the order identity holds for them all the same.)
Every start row s >= i0 is then valid too, which is how a lane follows its wave's row -- and how start row 1 is checked.

For every case the popped sequence of (row, column) of the full list merge must equal "the list merge of the rows below s alone,
G * s pops, then the rows s .. G-1 row by row", and the list the kernel carries -- all G heads -- must after G * s pops hold the
heads of the rows s .. G-1 in place at its front.  Cases: random operands at magnitude ratios 1 ... 1e-12 in both orientations,
constructed i0 = 2, G-2, G-1 and start row 1, the tie operands of the row-major model, k flat to 1e-9 with heads that
merge_init_order has to put in order (below the suffix; never in it), equal rows, leading zeros, G on both sides of every list
length with odd G * s.  No GPU: this pins the argument, tests/test_merge_suffix.py pins the kernel."""
import numpy as np
import pytest

from test_merge_rowmajor_model import lane_keys, list_len, random_operand, swap_choice, tie_operands

ALL_G = [8, 10, 12, 16, 17, 20, 32]
HUGE_BITS = 0x7FE0000000000000                   # the kernel's sentinel column: finite, above every optical depth
MIN_ROWS = [1, 2, 4]                             # the values of kSuffixMinRows the kernel was measured with
MIN_LIST = 16                                    # kSuffixMinList: shorter lists (G <= 10) keep the list to its end


def lane_i0(K):
    """merge_rowmajor_test for one lane: the running maximum of the rows' last keys against the next sorted head"""
    R = np.sort(K[:, 0])
    top = np.maximum.accumulate(K[:, -1])
    fails = np.nonzero(~(top[:-1] < R[1:]))[0]
    return 0 if fails.size == 0 else int(fails[-1]) + 2


def start_row(i0, G, min_rows, on=True):
    """merge_suffix_row: the row from which the merge is walked; G: the list to its end"""
    return i0 if i0 == 0 or (on and list_len(G) >= MIN_LIST and i0 <= G - min_rows) else G


def decode(key, swapped):
    low = key & 0x7FF
    return (low >> 6, low & 63) if swapped else (low & 31, low >> 5)


def list_pops(K, rows, npops, NR, swapped):
    """The register list over the heads of `rows` (sorted, as merge_init leaves them; unused entries "huge"): npops steps of
    pop R[0], insert the popped row's next key -- the sentinel of column G once the row is exhausted -- through the network
    t_0 = min(x, s_1), t_k = min(max(x, s_k), s_{k+1}), t_{NR-1} = max(x, s_{NR-1}).  Returns the popped (row, column) and the list."""
    G = K.shape[0]
    keys = [[int(v) for v in K[i]] for i in range(G)]
    for i in range(G):
        keys[i].append(HUGE_BITS | ((i << 6) | G if swapped else (G << 5) | i))
    R = sorted(keys[i][0] for i in rows) + [HUGE_BITS] * (NR - len(rows))
    out = []
    for t in range(npops):
        row, col = decode(R[0], swapped)
        assert col < G, "a sentinel was popped"
        out.append((row, col))
        x = keys[row][col + 1]
        mk = [max(x, R[k]) for k in range(1, NR - 1)]
        R[0] = min(x, R[1])
        for k in range(1, NR - 1):
            R[k] = min(mk[k - 1], R[k + 1])
        R[NR - 1] = max(x, R[NR - 1])
    return out, R


def steps_in_slots(nsteps):
    """k_ck_overlap's ping-pong over a list phase of nsteps steps: trips of (e0, e1) and, for an odd count, one more step on
    e0 -- the slot that holds the current element of every step, which must alternate from e0 whatever the parity"""
    slots = [0, 1] * (nsteps // 2) + ([0] if nsteps & 1 else [])
    assert slots == [t & 1 for t in range(nsteps)]
    return len(slots)


def check(K, swapped, i0=None, starts=None):
    """The full list's order against the partial form from every start row in `starts` (default: the lane's own i0, the
    last row)"""
    G = K.shape[0]
    NR = list_len(G)
    own = lane_i0(K)
    if i0 is not None:
        assert own == i0, (own, i0)
    full, _ = list_pops(K, range(G), G * G, NR, swapped)
    assert len(set(full)) == G * G
    if starts is None:
        starts = {own, G - 1}
    for s in sorted(starts):
        if not max(own, 1) <= s <= G:
            continue
        assert steps_in_slots(G * s) == G * s
        walked = [(i, j) for i in range(s, G) for j in range(G)]
        below, _ = list_pops(K, range(s), G * s, NR, swapped)
        assert below + walked == full, (G, s, swapped)
        # the kernel's list holds all G heads: the same pops, and the heads of the rows from s on are left in place
        part, R = list_pops(K, range(G), G * s, NR, swapped)
        assert part == below
        assert R[:G - s] == [int(v) for v in K[s:, 0]], (G, s, swapped)
    if own == 0:
        assert full == [(i, j) for i in range(G) for j in range(G)]
    return own


def gap_rows(G, i0):
    """Rows whose boundaries below i0 - 1 fail and from i0 - 1 on pass against columns that span 8: gaps of 1, then of 16"""
    gaps = np.where(np.arange(G - 1) < i0 - 1, 1.0, 16.0)
    return 1024.0 + np.concatenate([[0.0], np.cumsum(gaps)])


@pytest.mark.parametrize("G", ALL_G)
def test_random_operands(G):
    """Both orientations at every magnitude ratio; across them whole walks, suffixes and merges without one all occur, and a
    suffix of every admissible length class is taken by some kSuffixMinRows"""
    rng = np.random.default_rng(1700 + G)
    seen, taken = set(), set()
    for e in range(13):
        for _ in range(1 if G > 20 else 2 if G >= 16 else 8):    # short merges are cheap, and rarely without a suffix
            big, small = random_operand(rng, G), 10.0 ** -e * random_operand(rng, G)
            for a, b in ((big, small), (small, big)):
                sw = swap_choice(a, b)
                rows, cols = (b, a) if sw else (a, b)
                i0 = check(lane_keys(rows, cols, sw), sw)
                seen.add((sw, "whole" if i0 == 0 else "none" if i0 == G else "suffix"))
                taken |= {(m, 0 < start_row(i0, G, m) < G) for m in MIN_ROWS}
                assert start_row(i0, G, 1, on=False) in (0, G)
    assert seen == {(sw, kind) for sw in (False, True) for kind in ("whole", "suffix", "none")}, seen
    assert taken == {(m, t) for m in MIN_ROWS for t in ((False, True) if list_len(G) >= MIN_LIST else (False,))}


@pytest.mark.parametrize("target", ["1", "2", "G-2", "G-1"])
@pytest.mark.parametrize("G", ALL_G)
def test_constructed_start_rows(G, target):
    """i0 = 2, G-2 and G-1 by construction, in both orientations; 1 is not a value of the rule, so there every boundary passes
    (i0 = 0) and the partial form is checked from start row 1: row 0 through the list, G pops, then the walk.  G * i0 is odd
    for G = 17 with the odd rows among them."""
    i0 = {"1": 0, "2": 2, "G-2": G - 2, "G-1": G - 1}[target]
    r, c = gap_rows(G, i0), np.linspace(0.0, 8.0, G)
    for swapped in (False, True):
        a, b = (c, r) if swapped else (r, c)
        assert swap_choice(a, b) == swapped
        check(lane_keys(r, c, swapped), swapped, i0=i0, starts={1} if target == "1" else {i0, G - 1, G})
    if G == 17:
        assert (G * (G - 2)) & 1 and not (G * (G - 1)) & 1


@pytest.mark.parametrize("nudge", [0, 1, -1, 500])
@pytest.mark.parametrize("G", ALL_G)
def test_ties_across_the_row_boundary(G, nudge):
    """The row-major model's ties: every boundary ties in the top 53 bits, the packing decides -- all pass or all fail"""
    r, c = tie_operands(G, nudge)
    for swapped in (False, True):
        i0 = check(lane_keys(r, c, swapped), swapped, starts={1, 2, G - 2, G - 1})
        assert i0 == (0 if swapped or nudge < 0 else G), (G, nudge, swapped, i0)
    # ties below a suffix: the first boundaries tie, the others are wide open
    r2 = r.copy()
    r2[G // 2:] = r[G // 2 - 1] + 64.0 + 16.0 * np.arange(G - G // 2)
    for swapped in (False, True):
        i0 = check(lane_keys(r2, c, swapped), swapped)
        assert i0 == (0 if swapped or nudge < 0 else G // 2), (G, nudge, swapped, i0)


@pytest.mark.parametrize("G", ALL_G)
def test_flat_k_with_reordered_heads(G):
    """k flat to 1e-9 and a neighbouring pair of rows out of order beyond a key's precision, as a merged spectrum can be: the
    heads are not ascending, merge_init_order sorts them, and the suffix begins above the pair at the earliest -- the list
    phase pops the reordered rows correctly and the rows it leaves are in place.  Such a lane is never swapped."""
    seen = set()
    for span in (1e-9, 1e-8, 0.0):
        for i in (0, G // 2, G - 3, G - 2):
            rows = 3.0 * (1.0 + 1e-9 * np.arange(G))
            rows[i], rows[i + 1] = rows[i + 1], rows[i]
            cols = span * np.linspace(0.0, 1.0, G)
            assert not swap_choice(rows, cols + 4.0)
            K = lane_keys(rows, cols, False)
            assert K[i, 0] > K[i + 1, 0]
            i0 = check(K, False)
            assert i0 >= i + 2, (G, span, i, i0)
            seen.add("suffix" if i0 < G else "none")
    assert seen == {"suffix", "none"}


@pytest.mark.parametrize("G", ALL_G)
def test_equal_rows_and_leading_zeros(G):
    rng = np.random.default_rng(2100 + G)
    for ratio in (1.0, 1e-3, 1e-14, 0.0):
        rows = random_operand(rng, G) + 10.0
        rows[G // 2] = rows[G // 2 - 1]                                 # two equal neighbouring rows
        cols = ratio * random_operand(rng, G) if ratio else np.zeros(G)
        for sw in (False, True):
            check(lane_keys(rows, cols, sw), sw)
        zr, zc = random_operand(rng, G), ratio * random_operand(rng, G) if ratio else np.zeros(G)
        zr[:G // 2] = 0.0                                               # leading zeros in the rows, then in the columns too
        for sw in (False, True):
            check(lane_keys(zr, zc, sw), sw)
        zc[:G // 3] = 0.0
        for sw in (False, True):
            check(lane_keys(zr, zc, sw), sw)


@pytest.mark.parametrize("G", ALL_G)
def test_a_wave_follows_its_last_lane(G):
    """Lanes of both orientations with different i0: the wave takes the largest, and every lane's order is the partial form's
    from that row; one lane without a suffix takes it from all of them."""
    c = np.linspace(0.0, 8.0, G)
    lanes = [(gap_rows(G, i0), sw) for i0, sw in ((0, False), (2, True), (G // 2, False), (G - 2, True))]
    keys = [(lane_keys(r, c, sw), sw) for r, sw in lanes]
    wave = max(lane_i0(K) for K, _ in keys)
    assert wave == G - 2
    for K, sw in keys:
        check(K, sw, starts={wave})
    r, _ = tie_operands(G)
    assert max(wave, lane_i0(lane_keys(r, c, False))) == G
