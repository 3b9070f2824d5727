"""CPU simulation behind the tile cut along one wavenumber (the group width of LaneRow as run-time data): the r09
simulation's inputs, per-lane test (r09_merge_rowmajor_sim.row_major) and instruction model, with the lanes cut into tiles
(r08_merge_layer_groups_sim.tiles_of) of 4 wavenumbers x 16 rows, 2 x 32 and 1 x 64, a tile running on into the next wavenumber
group at the end of the 100 rows as the kernel's tiles do.  A wave walks a merge only when all 64 lanes pass the test, and its
list pass costs what its deepest lane needs.  Printed per cut:

  * the share of (tile, merge) pairs that walk, over all merges and merge by merge;
  * the fp64 list instructions per step in the tiles that keep the list (r06's pass cost at --bounds);
  * the estimate of wave64 VALU instructions per merged element, r09's model: the list path at its measured 33.1 with the
    simulated list cost taken out and put back per tile, the walk at 6;

and, as the bound no cut of whole waves reaches, the share of lanes that pass the test, and the share of wavenumbers whose 100
layers all agree in a given merge (how far "row-major or not" is a property of the wavenumber).

  python tools/experiments/r10_merge_one_wavenumber_sim.py [--waves 64] [--gases 8] [--ng 20] [--bounds 3,7,12] [--seed 20260704]

--waves must be a multiple of 16.  At the defaults: 22.9 / 29.4 / 35.9 % walking, 23.5 / 21.4 / 20.1 list instructions, estimates
31.8 / 28.1 / 25.2 (the figures this step was planned with read 31.9 / 28.2 / 25.3; where that tenth of an instruction comes from
was not found, the shares and list costs agree).  Regrouping the cells of a block between its merges is not simulated.
"""
import argparse
import importlib.util
import os

import numpy as np

_here = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("r09_sim", os.path.join(_here, "r09_merge_rowmajor_sim.py"))
r09 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(r09)
r08, r06, syn = r09.r08, r09.r06, r09.syn

WIDTHS = (4, 2, 1)


def lanes(W, G, S, L, seed):
    """(depth (S-1, W, L, steps), row-major (S-1, W, L, 1)) of every lane and merge: r09's loop, unchanged"""
    rng = np.random.default_rng(seed)
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
        rm.append(r09.row_major(rows, cols, swap))
        a_sorted = np.sort(a, axis=1)
        depth.append(r06.entry_depths(np.where(swap[:, None], b, a_sorted), np.where(swap[:, None], a_sorted, b)))
        sums = (a[:, :, None] + b[:, None, :]).reshape(N, G * G)
        order = np.argsort(sums, axis=1, kind="stable")
        a = r06.rebin(np.take_along_axis(sums, order, 1), wpair.reshape(-1)[order], g_ord)
    return np.stack(depth).reshape(S - 1, W, L, nsteps), np.stack(rm).reshape(S - 1, W, L, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waves", type=int, default=64)
    ap.add_argument("--gases", type=int, default=8)
    ap.add_argument("--ng", type=int, default=20)
    ap.add_argument("--bounds", default="3,7,12", help="kExitBounds of the list pass (r09's model: 3,7,12)")
    ap.add_argument("--seed", type=int, default=20260704)
    args = ap.parse_args()
    W, G, S, L = args.waves, args.ng, args.gases, 100
    bounds = tuple(int(b) for b in args.bounds.split(","))
    assert (W * L) % 64 == 0 and W % 16 == 0, "--waves: a multiple of 16"
    d, r = lanes(W, G, S, L, args.seed)
    print(f"bench family: {W} wavenumbers x {L} consecutive layers, G = {G}, {S} gases, exit bounds {bounds}")
    per_nu = r[..., 0].mean(axis=2)                             # (merge, wavenumber): share of the 100 layers that are row-major
    pure = (per_nu == 0.0) | (per_nu == 1.0)
    print(f"lanes that pass the test: {100.0 * r.mean():.1f} %   (merge, wavenumber) pairs whose {L} layers all agree: "
          f"{100.0 * pure.mean():.1f} %")
    print("cut (wavenumbers x rows) | (tile, merge) pairs that walk | list instructions per step, tiles that keep the list | "
          "est. VALU instructions per element | walking share, merge 1 .. %d" % (S - 1))
    cuts, other = [], None
    for nv in WIDTHS:
        dt, _ = r08.tiles_of(d, nv, W, L)                       # (merge, tile, 64, step)
        rt, _ = r08.tiles_of(r, nv, W, L)
        dm = dt.max(axis=-2)                                    # (merge, tile, step)
        tile_rm = rt[..., 0].all(axis=-1)                       # (merge, tile)
        keep = ~tile_rm
        list_keep = r06.pass_cost(dm[keep], bounds, G) if keep.any() else 0.0
        if nv == r09.NV:    # what is not the list pass (decode, repack, fetch, walk, branch): calibrated on the measured cut
            other = r09.MEASURED_PER_STEP - r06.pass_cost(dm, r09.BOUNDS, G)
        cuts.append((nv, tile_rm.mean(), list_keep, tile_rm.mean(axis=1)))
    for nv, share, list_keep, by_merge in cuts:
        est = (1.0 - share) * (other + list_keep) + share * r09.WALK_PER_STEP
        print(f"  {nv} x {64 // nv:2d} | {100.0 * share:5.1f} % | {list_keep:5.1f} | {est:5.1f} | "
              + " ".join(f"{v:.2f}" for v in by_merge))


if __name__ == "__main__":
    main()
