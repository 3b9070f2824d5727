"""CPU simulation behind the list-free walk of row-major merges (merge_rowmajor): the r08 simulation
(r08_merge_layer_groups_sim.py, whose inputs, tiles and crossing counts are used as they are, and through it r06's depths and
pass cost) with the kernel's test per lane and merge -- the last key of every row below the head of the next,
K(i, G-1) < K(i+1, 0), in the lane's own key packing -- and per tile of 2 wavenumbers x 32 rows (a wave walks a merge only when
all 64 lanes pass).  Printed:

  * the share of row-major merges per lane and per tile, for every merge and over all of them;
  * the re-entry depth d (0: the popped row's next key is the next winner), per lane and as the tile maximum;
  * the fp64 list instructions per step of the tiles that keep the list;
  * the estimate of wave64 VALU instructions per merged element: the list path at its measured 33.1 (r08: 1.546e9 per launch)
    with the simulated list cost taken out and put back per tile, the walk at 6 (two adds, the fma, the compare and the two
    instructions around the crossing branch).

  python tools/experiments/r09_merge_rowmajor_sim.py [--waves 32] [--gases 8] [--ng 20] [--seed 20260704]

--waves must make waves * 100 a multiple of 64 (16, 32, ...).
"""
import argparse
import importlib.util
import os

import numpy as np

_here = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("r08_sim", os.path.join(_here, "r08_merge_layer_groups_sim.py"))
r08 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(r08)
r06, syn = r08.r06, r08.syn

BOUNDS = (3, 7, 12)            # kExitBounds
MEASURED_PER_STEP = 33.1       # wave64 VALU instructions per merged element of the parent kernel at C2 (profiles/r08)
WALK_PER_STEP = 6.0
NV = 2                         # kLaneNV


def row_major(rows, cols, swapped):
    """(N,) bool: merge_rowmajor_test.  rows, cols (N, G); the keys as 64-bit patterns, low 11 bits (col << 5) | row or, in a
    swapped lane, (row << 6) | col; the heads sorted as merge_init leaves them."""
    N, G = rows.shape
    i = np.arange(G, dtype=np.uint64)[None, :]
    sw = swapped[:, None]
    top = lambda v: np.ascontiguousarray(v).view(np.uint64) & ~np.uint64(0x7FF)
    heads = top(rows + cols[:, :1]) | np.where(sw, i << np.uint64(6), i)
    lasts = top(rows + cols[:, -1:]) | np.where(sw, (i << np.uint64(6)) | np.uint64(G - 1), (np.uint64(G - 1) << np.uint64(5)) | i)
    heads = np.sort(heads, axis=1)
    return np.all(lasts[:, :-1] < heads[:, 1:], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waves", type=int, default=32)
    ap.add_argument("--gases", type=int, default=8)
    ap.add_argument("--ng", type=int, default=20)
    ap.add_argument("--seed", type=int, default=20260704)
    args = ap.parse_args()
    W, G, S, L = args.waves, args.ng, args.gases, 100
    assert (W * L) % 64 == 0 and W % 8 == 0, "--waves: a multiple of 16"
    rng = np.random.default_rng(args.seed)
    atm = syn.synth_atmosphere(L, S, seed=7)
    p_bar, temp, amount = atm["lay_press_pa"][0] / 1e5, atm["lay_temp"][0], atm["amount"][0]
    _, delg = syn.gauss_legendre_01(G, as_float32=True)
    dg = delg.astype(np.float32)
    wpair = (dg[:, None] * dg[None, :]).astype(np.float64)
    g_ord = np.concatenate([[0.0], np.cumsum(dg).astype(np.float64)])
    g_ord[G] = 1.0
    tau = r06.bench_family_k(rng, W, G, S, p_bar, temp) * amount.T[None, :, :, None]     # (W, L, S, G)
    N, nsteps = W * L, G * G - G + 1
    a = tau[:, :, 0].reshape(N, G)
    depth, rm = [], []
    for s in range(1, S):
        b = tau[:, :, s].reshape(N, G)
        swap = (b[:, -1] > a[:, -1]) & np.all(np.diff(a, axis=1) >= 0.0, axis=1)
        rows, cols = np.where(swap[:, None], b, a), np.where(swap[:, None], a, b)
        rm.append(row_major(rows, cols, swap))
        a_sorted = np.sort(a, axis=1)
        depth.append(r06.entry_depths(np.where(swap[:, None], b, a_sorted), np.where(swap[:, None], a_sorted, b)))
        sums = (a[:, :, None] + b[:, None, :]).reshape(N, G * G)
        order = np.argsort(sums, axis=1, kind="stable")
        w_sorted = wpair.reshape(-1)[order]
        a = r06.rebin(np.take_along_axis(sums, order, 1), w_sorted, g_ord)
    d = np.stack(depth).reshape(S - 1, W, L, nsteps)
    r = np.stack(rm).reshape(S - 1, W, L, 1)
    dt, _ = r08.tiles_of(d, NV, W, L)                           # (merge, tile, 64, step)
    rt, _ = r08.tiles_of(r, NV, W, L)
    dm = dt.max(axis=-2)                                        # (merge, tile, step)
    tile_rm = rt[..., 0].all(axis=-1)                           # (merge, tile)
    print(f"bench family: {W} wavenumbers x {L} consecutive layers, G = {G}, {S} gases, tiles of {NV} wavenumbers x {64 // NV} rows")
    print(f"re-entry depth d = 0 in {100.0 * (d == 0).mean():.0f} % of a lane's steps, the tile maximum in "
          f"{100.0 * (dm == 0).mean():.0f} % of steps")
    print("row-major merges, merge s = 1 .. %d:" % (S - 1))
    print("  lanes: " + " ".join(f"{v:.2f}" for v in r.mean(axis=(1, 2, 3))) + f"   all: {100.0 * r.mean():.0f} %")
    print("  tiles: " + " ".join(f"{v:.2f}" for v in tile_rm.mean(axis=1)) + f"   all: {100.0 * tile_rm.mean():.0f} %")
    list_all = r06.pass_cost(dm, BOUNDS, G)
    keep = ~tile_rm
    list_keep = r06.pass_cost(dm[keep], BOUNDS, G) if keep.any() else 0.0
    other = MEASURED_PER_STEP - list_all                        # decode, repack, fetch, walk, branch: what is not the pass
    share = tile_rm.mean()
    est = (1.0 - share) * (other + list_keep) + share * WALK_PER_STEP
    print(f"fp64 list instructions per step: {list_all:.1f} over all tiles, {list_keep:.1f} in the tiles that keep the list")
    print(f"wave64 VALU instructions per merged element: {MEASURED_PER_STEP:.1f} -> {est:.1f} "
          f"({100.0 * (est / MEASURED_PER_STEP - 1.0):+.0f} %) with the walk at {WALK_PER_STEP:.0f}")


if __name__ == "__main__":
    main()
