"""A model in plain Python of the two trims of the forward merge's list pass (kMergeExit, kMergeOrient in
csrc/ansfm_merge64.hip.h): a "wave" of a few register lists stepped together,
  * the pass in chunks that end at compile-time boundaries, left at the first boundary c with no lane's x above R[c]
    (merge_pass_exit), with the peeled tail of merge_peel on top, and
  * per lane, the rows taken from the operand with the larger top ordinate, the low 11 key bits of a swapped lane packed as
    (row << 6) | col instead of (col << 5) | row (MergeOrient),
against the full pass over the unswapped list, lane by lane: the sequence of popped (a-index, b-index) pairs must be the same,
for every G of every instantiated list length -- random input, one operand 1e6 times the other either way, input flat to 1e-9
(keys that tie: the low bits decide), and an `a` with one neighbour pair out of order, which must refuse the swap.
No GPU: this pins the argument, tests/test_merge_exit_orient.py pins the kernel."""
import random
import struct

import pytest

HUGE = struct.unpack('<d', struct.pack('<Q', 0x7FE0000000000000))[0]
LANES = 4


def _bits(v):
    """A key is kept as the 64-bit pattern of its double: non-negative doubles compare like their patterns, so the lists below
    hold integers and v_min_f64 / v_max_f64 are min / max of them."""
    return struct.unpack('<Q', struct.pack('<d', v))[0]


class Lane:
    """One lane's operands the way the kernel addresses them: rows, columns (with the sentinel column G), the bit offsets of
    the two key fields and the increment that steps the column."""

    def __init__(self, a, b, swapped):
        self.swapped = swapped
        self.rows, cols = (b, a) if swapped else (a, b)
        self.cols = list(cols) + [HUGE, 0.0]
        self.rsh, self.csh, self.inc = (6, 0, 1) if swapped else (0, 5, 32)

    def pack_head(self, i):
        return (_bits(self.rows[i] + self.cols[0]) & ~0x7FF) | (i << self.rsh)

    def fetch(self, key):
        kb = key & 0xFFFFFFFF
        ci, cp = (kb >> self.rsh) & 31, (kb >> self.csh) & 63
        return dict(kw=kb, ci=ci, cp=cp, ai=self.rows[ci] if ci < len(self.rows) else 0.0, bc=self.cols[cp], bn=self.cols[cp + 1])

    def next_key(self, e):                     # pack_key11_next with the per-lane increment
        b = _bits(e['ai'] + e['bn'])
        return (b & ~0x7FF) | ((e['kw'] + self.inc) & 0x7FF)

    def pair(self, e):                         # (a-index, b-index) of a popped element
        return (e['cp'], e['ci']) if self.swapped else (e['ci'], e['cp'])


def swap_choice(a, b):
    """The kernel's criterion: rows = the operand with the larger top ordinate; b only where a is non-decreasing."""
    return b[-1] > a[-1] and all(a[g + 1] >= a[g] for g in range(len(a) - 1))


BOUNDS = (4, 10)                               # kExitBounds (ansfm_merge64.hip.h) as committed
OTHER_BOUNDS = [(4, 8, 12, 16, 20, 24, 28), (2, 5, 9, 14, 20, 27), (3, 7, 12, 18, 25), (8,)]


def exit_bound(k0, kind):
    """merge_exit_bound: the first chunk boundary above k0 in the ascending list `kind`, none: beyond every list."""
    return next((b for b in kind if b > k0), 1000)


def init_list(ln, G, NR):
    R = [ln.pack_head(i) if i < G else _bits(HUGE) for i in range(NR)]
    return sorted(R)                           # merge_init puts heads in order when some lane's are not


def full_step(R, x, NP):
    """merge_step's pass without the exit."""
    if NP == 1:
        R[0] = x
        return
    R[0] = min(x, R[1])
    mk = [max(x, R[k]) for k in range(1, NP - 1)]
    for j, k in enumerate(range(1, NP - 1)):
        R[k] = min(mk[j], R[k + 1])
    R[NP - 1] = max(x, R[NP - 1])


def exit_step(Rs, xs, NP, kind, depth):
    """The pass of every lane of the wave with merge_pass_exit: chunks [K0, K1), the wave-level test between them."""
    if NP == 1:
        for R, x in zip(Rs, xs):
            R[0] = x
        return
    for R, x in zip(Rs, xs):
        R[0] = min(x, R[1])
    k0 = 1
    while True:
        k1 = exit_bound(k0, kind) if exit_bound(k0, kind) < NP - 2 else NP - 1
        for R, x in zip(Rs, xs):
            mk = [max(x, R[k]) for k in range(k0, k1)]
            for j, k in enumerate(range(k0, k1)):
                R[k] = min(mk[j], R[k + 1])
        if k1 == NP - 1:
            for R, x in zip(Rs, xs):
                R[NP - 1] = max(x, R[NP - 1])
            depth.append(NP)
            return
        if not any(x > R[k1] for R, x in zip(Rs, xs)):
            depth.append(k1)
            return
        k0 = k1


def run_reference(a, b, G, NR):
    """One lane, unswapped, full-length passes throughout."""
    ln = Lane(a, b, False)
    R = init_list(ln, G, NR)
    e = ln.fetch(R[0])
    out = []
    for _ in range(G * G):
        full_step(R, ln.next_key(e), NR)
        out.append(ln.pair(e))
        e = ln.fetch(R[0])
    return out


def run_wave(As, Bs, G, NR, kind, orient=True):
    lanes = [Lane(a, b, orient and swap_choice(a, b)) for a, b in zip(As, Bs)]
    Rs = [init_list(ln, G, NR) for ln in lanes]
    es = [ln.fetch(R[0]) for ln, R in zip(lanes, Rs)]
    outs = [[] for _ in lanes]
    depth = []

    def do(NP):
        nonlocal es
        exit_step(Rs, [ln.next_key(e) for ln, e in zip(lanes, es)], NP, kind, depth)
        for ln, e, o in zip(lanes, es, outs):
            o.append(ln.pair(e))
        if NP > 1:
            es = [ln.fetch(R[0]) for ln, R in zip(lanes, Rs)]
    for _ in range(G * G - (G - 1)):
        do(NR)
    for NP in range(NR - 1, 0, -1):            # merge_peel
        if NP < G:
            do(NP)
    return outs, [ln.swapped for ln in lanes], depth


def _sorted_random(G, lo, hi):
    return sorted(10 ** random.uniform(lo, hi) for _ in range(G))


def _flat(G, base):
    return [base * (1.0 + g * 1e-9 / G) for g in range(G)]


def _wave_inputs(G, case):
    """LANES (a, b) pairs of one wave; every case mixes lanes of both orientations where its inputs allow it."""
    As, Bs = [], []
    for lane in range(LANES):
        if case == "random":
            a, b = _sorted_random(G, -3, 2), _sorted_random(G, -3, 2)
        elif case == "b_dominates":
            a, b = _sorted_random(G, -3, 2), [1e6 * v for v in _sorted_random(G, -3, 2)]
        elif case == "a_dominates":
            a, b = [1e6 * v for v in _sorted_random(G, -3, 2)], _sorted_random(G, -3, 2)
        elif case == "mixed":
            a, b = _sorted_random(G, -3, 2), _sorted_random(G, -3, 2)
            if lane % 2:
                b = [1e6 * v for v in b]
            else:
                a = [1e6 * v for v in a]
        elif case == "flat":
            a, b = _flat(G, 10 ** random.uniform(-2, 1)), _flat(G, 10 ** random.uniform(-2, 1))
        elif case == "flat_zeros":
            a, b = _flat(G, 10 ** random.uniform(-2, 1)), _flat(G, 10 ** random.uniform(-2, 1))
            (a if lane % 2 else b)[:G // 2] = [0.0] * (G // 2)
        else:
            raise ValueError(case)
        As.append(a)
        Bs.append(b)
    return As, Bs


CASES = ["random", "b_dominates", "a_dominates", "mixed", "flat", "flat_zeros"]


@pytest.mark.parametrize("NR", [8, 10, 16, 20, 32])
def test_exit_and_orientation_pop_the_unswapped_full_pass_order(NR):
    random.seed(100 + NR)
    swapped_lanes = kept_lanes = 0
    for G in range(1, NR + 1):
        for case in CASES:
            As, Bs = _wave_inputs(G, case)
            refs = [run_reference(a, b, G, NR) for a, b in zip(As, Bs)]
            for ref in refs:
                assert len(ref) == G * G and len(set(ref)) == G * G
            outs, swapped, _ = run_wave(As, Bs, G, NR, kind=BOUNDS)
            assert outs == refs, (NR, G, case, swapped)
            swapped_lanes += sum(swapped)
            kept_lanes += len(swapped) - sum(swapped)
            # the exit alone, every lane as the kernel orients it without kMergeOrient
            outs, swapped, _ = run_wave(As, Bs, G, NR, kind=BOUNDS, orient=False)
            assert outs == refs and not any(swapped), (NR, G, case)
    assert swapped_lanes > 0 and kept_lanes > 0


@pytest.mark.parametrize("kind", OTHER_BOUNDS)
@pytest.mark.parametrize("NR", [8, 20, 32])
def test_other_chunk_boundaries(NR, kind):
    random.seed(200 + 10 * NR + len(kind))
    for G in range(1, NR + 1):
        for case in ("mixed", "flat"):
            As, Bs = _wave_inputs(G, case)
            refs = [run_reference(a, b, G, NR) for a, b in zip(As, Bs)]
            outs, _, _ = run_wave(As, Bs, G, NR, kind=kind)
            assert outs == refs, (NR, G, case, kind)


@pytest.mark.parametrize("NR", [8, 10, 16, 20, 32])
def test_a_with_a_swapped_neighbour_pair_refuses_the_swap(NR):
    """A merged spectrum can have two neighbours that the rounding of the bin averages has put out of order: such an `a` cannot
    be the columns, whatever its size against b.  The lane keeps today's orientation (and merge_init orders its heads)."""
    random.seed(300 + NR)
    for G in range(2, NR + 1):
        As, Bs = _wave_inputs(G, "b_dominates")
        j = random.randrange(G - 1)
        a = _flat(G, 0.5)
        a[j], a[j + 1] = a[j + 1], a[j]
        assert a[j] > a[j + 1] and Bs[2][-1] > a[-1]
        As[2] = a
        outs, swapped, _ = run_wave(As, Bs, G, NR, kind=BOUNDS)
        assert swapped == [True, True, False, True], (NR, G, swapped)
        refs = [run_reference(x, y, G, NR) for x, y in zip(As, Bs)]
        assert outs == refs, (NR, G)


def test_the_orientation_shortens_the_pass_where_b_dominates():
    """What the choice is for: with b 1e6 times a the unswapped pass runs to the end of the list in most steps, the swapped one
    ends at the first boundary in most."""
    random.seed(7)
    G = NR = 20
    As, Bs = _wave_inputs(G, "b_dominates")
    _, _, deep = run_wave(As, Bs, G, NR, kind=BOUNDS, orient=False)
    _, swapped, shallow = run_wave(As, Bs, G, NR, kind=BOUNDS)
    assert all(swapped)
    main = G * G - (G - 1)
    mean = lambda d: sum(d[:main]) / main
    print(f"mean pass length over the {main} full-list steps: unswapped {mean(deep):.1f}, swapped {mean(shallow):.1f}")
    assert mean(shallow) < 0.5 * mean(deep)
