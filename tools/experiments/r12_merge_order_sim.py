"""CPU simulation behind the wavenumber order of the forward merge (merge_order_inverse): r10's lanes and
instruction model at the committed cut (1 wavenumber x 64 rows, a tile running on into the next wavenumber at the end of the
100 rows), with the 64 wavenumbers of a block handed out in another order.  "Row-major or not" is a property of the wavenumber,
so a tile that straddles two wavenumbers walks when they are two of a kind: the block is sorted (stably, so equal patterns keep
their wavenumber order) by the pattern byte of a wavenumber, its verdicts of merges 1 .. 8 at one row, merge 1 most significant.
In the kernel the byte comes from the launch before; here it is taken from the same lanes, which is what a launch on the same
table and nearly the same atmosphere sees.  Printed per order, as r10 prints per cut:

  * the share of (tile, merge) pairs that walk;
  * the fp64 list instructions per step in the tiles that keep the list;
  * the estimate of wave64 VALU instructions per merged element (r09's model, calibrated as in r10);

for the committed order, each block sorted by the pattern of row R / 2 and of row 0, the same with 10 % of the bytes replaced by
random ones (a stale hint), and a random order in each block (a useless hint: what the sort costs when it knows nothing).

  python tools/experiments/r12_merge_order_sim.py [--waves 256] [--gases 8] [--ng 20] [--bounds 2,6,11] [--seed 20260704]

--waves must be a multiple of 64.
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

BLOCK = 64


def pattern_bytes(r, row):
    """(W,) the byte a launch writes per wavenumber: the verdicts of merges 1 .. 8 at `row`, merge 1 in bit 7"""
    byte = np.zeros(r.shape[1], dtype=np.int64)
    for m in range(min(8, r.shape[0])):
        byte |= r[m, :, row, 0].astype(np.int64) << (7 - m)
    return byte


def block_order(byte):
    """(W,) the wavenumber at each position: every block of 64 sorted by (byte, wavenumber), the kernel's key"""
    W = byte.shape[0]
    key = (byte << 6) | (np.arange(W) % BLOCK)
    return np.concatenate([b + np.argsort(key[b:b + BLOCK], kind="stable") for b in range(0, W, BLOCK)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waves", type=int, default=256)
    ap.add_argument("--gases", type=int, default=8)
    ap.add_argument("--ng", type=int, default=20)
    ap.add_argument("--bounds", default="2,6,11", help="kExitBounds of the list pass")
    ap.add_argument("--seed", type=int, default=20260704)
    args = ap.parse_args()
    W, G, S, L = args.waves, args.ng, args.gases, 100
    bounds = tuple(int(b) for b in args.bounds.split(","))
    assert W % BLOCK == 0, "--waves: a multiple of 64"
    d, r = r10.lanes(W, G, S, L, args.seed)
    rng = np.random.default_rng(args.seed + 1)
    print(f"bench family: {W} wavenumbers x {L} consecutive layers, G = {G}, {S} gases, exit bounds {bounds}")
    print(f"lanes that pass the test: {100.0 * r.mean():.1f} %")

    # what is not the list pass, calibrated on the measured cut as in r10
    dt, _ = r08.tiles_of(d, r09.NV, W, L)
    other = r09.MEASURED_PER_STEP - r06.pass_cost(dt.max(axis=-2), r09.BOUNDS, G)

    mid, first = pattern_bytes(r, L // 2), pattern_bytes(r, 0)
    stale = mid.copy()
    wrong = rng.random(W) < 0.10
    stale[wrong] = rng.integers(0, 256, int(wrong.sum())) & (0xFF00 >> min(8, S - 1) & 0xFF)
    orders = (("as committed", np.arange(W)),
              (f"block sorted by the pattern of row {L // 2}", block_order(mid)),
              ("block sorted by the pattern of row 0", block_order(first)),
              (f"row {L // 2}, 10 % of the hints random", block_order(stale)),
              ("random order in each block", block_order(rng.integers(0, 256, W))))
    print("order | (tile, merge) pairs that walk | list instructions per step, tiles that keep the list | "
          "est. VALU instructions per element")
    base = None
    for name, perm in orders:
        assert sorted(perm.tolist()) == list(range(W))
        dt, _ = r08.tiles_of(d[:, perm], 1, W, L)               # (merge, tile, 64, step)
        rt, _ = r08.tiles_of(r[:, perm], 1, W, L)
        tile_rm = rt[..., 0].all(axis=-1)                       # (merge, tile)
        keep = ~tile_rm
        list_keep = r06.pass_cost(dt.max(axis=-2)[keep], bounds, G) if keep.any() else 0.0
        share = tile_rm.mean()
        est = (1.0 - share) * (other + list_keep) + share * r09.WALK_PER_STEP
        base = est if base is None else base
        print(f"  {name:45s} | {100.0 * share:5.1f} % | {list_keep:5.1f} | {est:6.2f} ({100.0 * (est / base - 1.0):+.1f} %)")


if __name__ == "__main__":
    main()
