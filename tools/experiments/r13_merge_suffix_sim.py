"""CPU simulation behind the walk of the separable top rows of a list merge (merge_suffix_row): r10's inputs and loop
(r10_merge_one_wavenumber_sim.lanes, unchanged -- its call of r09's per-lane test is wrapped to keep every lane's i0 as well),
the kernel's own rule on the 11-bit keys with sorted heads (boundary i passes when the largest last key of the rows 0 .. i is
below the next head; i0 = the last failing boundary + 2, or 0), and tiles of 1 wavenumber x 64 rows in wavenumber order.  A tile
takes the largest i0 of its lanes; with 0 < i0 <= G - kSuffixMinRows it runs the list for G * i0 elements and walks the rest.

Printed: the share of (tile, merge) pairs that walk whole; of the list tiles, the share with a suffix of at least one row and the
histogram of the suffix length G - i0; the share of the list tiles' rows, and of all merged elements, that lie in a suffix; and
per kSuffixMinRows in 1, 2, 4 the modelled wave64 VALU instructions per merged element before and after.  The model is r09's /
r10's: a walked element costs 6, a list element what is not the list pass (calibrated as in r10: r09's measured 33.1 less the
simulated pass cost of the cut it was measured on) plus the pass cost of its own step at --bounds; the test's extra compare
and maximum per row are added per merge.  The peeled last G - 1 steps of a list merge are not simulated (r06): a suffix step
among them is counted at the pass cost of the step before the peel.

  python tools/experiments/r13_merge_suffix_sim.py [--waves 64] [--gases 8] [--ng 20] [--bounds 2,6,11] [--seed 20260704]
"""
import argparse
import importlib.util
import os

import numpy as np

_here = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("r10_sim", os.path.join(_here, "r10_merge_one_wavenumber_sim.py"))
r10 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(r10)
r09, r08, r06 = r10.r09, r10.r08, r10.r06

MIN_ROWS = (1, 2, 4)
TEST_EXTRA_PER_ROW = 2.0       # v_max_f64 and the scalar code of one boundary, per merge and row


def lane_i0(rows, cols, swapped):
    """(N,) int: merge_rowmajor_test's row for every lane.  The keys as in r09.row_major."""
    N, G = rows.shape
    i = np.arange(G, dtype=np.uint64)[None, :]
    sw = swapped[:, None]
    top = lambda v: np.ascontiguousarray(v).view(np.uint64) & ~np.uint64(0x7FF)
    heads = top(rows + cols[:, :1]) | np.where(sw, i << np.uint64(6), i)
    lasts = top(rows + cols[:, -1:]) | np.where(sw, (i << np.uint64(6)) | np.uint64(G - 1), (np.uint64(G - 1) << np.uint64(5)) | i)
    heads = np.sort(heads, axis=1)
    fails = ~(np.maximum.accumulate(lasts, axis=1)[:, :-1] < heads[:, 1:])
    last_fail = (G - 2) - np.argmax(fails[:, ::-1], axis=1)
    return np.where(fails.any(axis=1), last_fail + 2, 0)


def lanes_with_i0(W, G, S, L, seed):
    """r10.lanes and, beside its two arrays, i0 (S-1, W, L, 1): the loop is r10's, r09.row_major is wrapped for the call"""
    kept, plain = [], r09.row_major

    def wrapped(rows, cols, swapped):
        kept.append(lane_i0(rows, cols, swapped))
        return plain(rows, cols, swapped)
    r09.row_major = wrapped
    try:
        d, r = r10.lanes(W, G, S, L, seed)
    finally:
        r09.row_major = plain
    i0 = np.stack(kept).reshape(S - 1, W, L, 1)
    assert np.array_equal(i0[..., 0] == 0, r[..., 0]), "i0 = 0 is r09's verdict"
    return d, r, i0


def step_costs(dm, bounds, G):
    """fp64 list instructions of every step (r06.pass_cost without the mean)"""
    full = 2 * G - 2
    cost = np.full(dm.shape, float(full + len(bounds)))
    done = np.zeros(dm.shape, dtype=bool)
    for n, c in enumerate(bounds):
        hit = ~done & (dm < c)
        cost[hit] = 1 + 2 * (c - 1) + (n + 1)
        done |= hit
    return cost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waves", type=int, default=64)
    ap.add_argument("--gases", type=int, default=8)
    ap.add_argument("--ng", type=int, default=20)
    ap.add_argument("--bounds", default="2,6,11", help="kExitBounds of the list pass")
    ap.add_argument("--seed", type=int, default=20260704)
    args = ap.parse_args()
    W, G, S, L = args.waves, args.ng, args.gases, 100
    bounds = tuple(int(b) for b in args.bounds.split(","))
    assert (W * L) % 64 == 0 and W % 16 == 0, "--waves: a multiple of 16"
    d, r, i0 = lanes_with_i0(W, G, S, L, args.seed)
    print(f"bench family: {W} wavenumbers x {L} consecutive layers, G = {G}, {S} gases, exit bounds {bounds}, tiles 1 x 64")
    # what is not the list pass, calibrated on the cut and bounds the 33.1 was measured with (r10)
    dcal, _ = r08.tiles_of(d, r09.NV, W, L)
    other = r09.MEASURED_PER_STEP - r06.pass_cost(dcal.max(axis=-2), r09.BOUNDS, G)
    dt, _ = r08.tiles_of(d, 1, W, L)                            # (merge, tile, 64, step)
    it, _ = r08.tiles_of(i0, 1, W, L)
    dm = dt.max(axis=-2)                                        # (merge, tile, step): the main-loop steps 0 .. G*G - G
    ti0 = it[..., 0].max(axis=-1)                               # (merge, tile)
    walk = ti0 == 0
    listed = ~walk
    cost = step_costs(dm, bounds, G)
    cost = np.concatenate([cost, np.repeat(cost[..., -1:], G - 1, axis=-1)], axis=-1)     # the peeled steps: see above
    assert cost.shape[-1] == G * G
    suffix = np.where(listed, G - ti0, 0)                       # rows
    print(f"(tile, merge) pairs that walk whole: {100.0 * walk.mean():.1f} %")
    print(f"list tiles with a suffix of at least one row: {100.0 * (suffix[listed] > 0).mean():.1f} %   "
          f"their rows in a suffix: {100.0 * suffix[listed].mean() / G:.1f} %   of all merged elements: {100.0 * suffix.mean() / G:.1f} %")
    hist = np.bincount(suffix[listed], minlength=G)
    print("suffix length (rows) : share of list tiles, %")
    print("  " + "  ".join(f"{n}:{100.0 * h / listed.sum():.1f}" for n, h in enumerate(hist)))
    list_el = other + cost                                      # per element of a list tile, by step
    before = (walk.mean() * r09.WALK_PER_STEP * G * G + (list_el * listed[..., None]).sum() / walk.size) / (G * G)
    print(f"not the list pass: {other:.1f} per element; list pass {cost[listed].mean():.1f} per step in the list tiles; "
          f"modelled instructions per element before: {before:.2f}")
    step = np.arange(G * G)[None, None, :]
    for m in MIN_ROWS:
        start = np.where(listed & (ti0 <= G - m), ti0, G)       # the first row walked; G: none
        walked_el = listed[..., None] & (step >= (G * start)[..., None])
        saved = ((list_el - r09.WALK_PER_STEP) * walked_el).sum() / walk.size / (G * G)
        after = before - saved + TEST_EXTRA_PER_ROW * (G - 1) / (G * G)
        print(f"kSuffixMinRows = {m}: elements walked behind a list phase {100.0 * walked_el.mean():.1f} % of all; "
              f"instructions per element {before:.2f} -> {after:.2f} ({100.0 * (after / before - 1.0):+.1f} %)")


if __name__ == "__main__":
    main()
