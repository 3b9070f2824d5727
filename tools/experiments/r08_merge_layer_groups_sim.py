"""CPU simulation behind the layer-grouped lanes of the forward merge (LaneRow): the r06 simulation
(r06_merge_exit_orient_sim.py, whose inputs, depths and pass cost are used as they are) with the tiles cut exactly as the
kernel cuts them -- the cells of a wavenumber block numbered (wavenumber / NV, row, wavenumber % NV), 64 consecutive cells per
tile, all 100 consecutive layers of the bench atmosphere as the row axis -- and two more figures per grouping:

  * how often some lane of the tile closes a bin in a step (the crossing branch of merge_walk_nodiv is wave-uniform: it is
    entered when any lane crosses);
  * the seam: tiles that run on into the next wavenumber group (100 rows are not a multiple of 64 / NV) against tiles that
    lie inside one group.

  python tools/experiments/r08_merge_layer_groups_sim.py [--waves 16] [--ng 20] [--gases 8]

--waves must make waves * 100 a multiple of 64 (16, 32, ...).  Rows = the larger operand (kMergeOrient), as the kernel runs.
"""
import argparse
import importlib.util
import os

import numpy as np

_here = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("r06_sim", os.path.join(_here, "r06_merge_exit_orient_sim.py"))
r06 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(r06)
syn = r06.syn


def crossings(w_sorted, g_ord, nsteps):
    """(N, nsteps) bool: the element consumed in step t carries the running weight sum over a bin boundary"""
    cum = np.cumsum(w_sorted, axis=1)
    nb = np.searchsorted(g_ord[1:-1], cum.reshape(-1), side="right").reshape(cum.shape)    # boundaries at or below the sum
    before = np.concatenate([np.zeros((cum.shape[0], 1), dtype=nb.dtype), nb[:, :-1]], axis=1)
    return (nb > before)[:, :nsteps]


def tiles_of(x, nv, W, L):
    """x: (..., W, L, steps) -> (..., tiles, 64, steps) in the kernel's cell order, and per tile whether it spans two groups"""
    lead = x.shape[:-3]
    y = x.reshape(lead + (W // nv, nv, L, x.shape[-1]))
    y = np.moveaxis(y, -3, -2)                                  # (..., group, row, w % nv, steps)
    y = y.reshape(lead + (W * L // 64, 64, x.shape[-1]))
    first = np.arange(W * L // 64) * (64 // nv)                 # first (group, row) pair of every tile
    seam = first // L != (first + 64 // nv - 1) // L
    return y, seam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waves", type=int, default=16)
    ap.add_argument("--ng", type=int, default=20)
    ap.add_argument("--gases", type=int, default=8)
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
    depth, cross = [], []
    for s in range(1, S):
        b = tau[:, :, s].reshape(N, G)
        swap = (b[:, -1] > a[:, -1]) & np.all(np.diff(a, axis=1) >= 0.0, axis=1)
        a_sorted = np.sort(a, axis=1)
        depth.append(r06.entry_depths(np.where(swap[:, None], b, a_sorted), np.where(swap[:, None], a_sorted, b)))
        sums = (a[:, :, None] + b[:, None, :]).reshape(N, G * G)
        order = np.argsort(sums, axis=1, kind="stable")
        w_sorted = wpair.reshape(-1)[order]
        cross.append(crossings(w_sorted, g_ord, nsteps))
        a = r06.rebin(np.take_along_axis(sums, order, 1), w_sorted, g_ord)
    d = np.stack(depth).reshape(S - 1, W, L, nsteps)
    c = np.stack(cross).reshape(S - 1, W, L, nsteps)
    print(f"bench family: {W} wavenumbers x {L} consecutive layers, G = {G}, {S} gases, {nsteps} main-loop steps per merge; "
          f"a lane closes a bin in {100.0 * c.mean():.1f} % of its steps")
    bound_sets = [(4, 10), (3, 9), (3, 7, 12), (2, 5, 9, 14)]
    # today's wave: 64 wavenumbers of one layer (needs 64 wavenumbers; with fewer, the wavenumbers there are)
    wv = min(W, 64)
    dm = d.reshape(S - 1, W // wv, wv, L, nsteps).max(axis=2)
    cm = c.reshape(S - 1, W // wv, wv, L, nsteps).any(axis=2)
    costs = ", ".join(f"{'/'.join(map(str, bs))}: {r06.pass_cost(dm, bs, G):.1f}" for bs in bound_sets)
    print(f"{wv} wavenumbers x 1 layer: mean of max d {dm.mean():.1f}; some lane closes a bin in {100.0 * cm.mean():.0f} % of "
          f"steps; fp64 list instructions per step: {costs}")
    for nv in (8, 4, 2):
        dt, seam = tiles_of(d, nv, W, L)
        ct, _ = tiles_of(c, nv, W, L)
        dm, cm = dt.max(axis=-2), ct.any(axis=-2)                # (merge, tile, step)
        costs = ", ".join(f"{'/'.join(map(str, bs))}: {r06.pass_cost(dm, bs, G):.1f}" for bs in bound_sets)
        print(f"{nv} wavenumbers x {64 // nv} rows: mean of max d {dm.mean():.1f}; some lane closes a bin in "
              f"{100.0 * cm.mean():.0f} % of steps; fp64 list instructions per step: {costs}")
        if seam.any() and not seam.all():
            inside, across = dm[:, ~seam], dm[:, seam]
            print(f"    seam: {int(seam.sum())} of {seam.size} tiles run into the next wavenumber group; 4/10 cost "
                  f"{r06.pass_cost(across, (4, 10), G):.1f} in them against {r06.pass_cost(inside, (4, 10), G):.1f} in the others "
                  f"(mean of max d {across.mean():.1f} against {inside.mean():.1f})")


if __name__ == "__main__":
    main()
