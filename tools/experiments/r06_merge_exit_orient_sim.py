"""CPU simulation behind kMergeExit / kMergeOrient: where the popped row's next key re-enters the
sorted list of the forward merge, per lane and as the maximum over the lanes that step together, for the bench family.

  python tools/experiments/r06_merge_exit_orient_sim.py [--waves 64] [--layers 5] [--ng 20] [--gases 8]

Inputs: the recipe of bench.py's torch_ktable with the NumPy RNG (k = base * shape(g) * p^pexp * (T / 200)^texp, evaluated at
the layer's own p, T instead of interpolated from the grid), the amounts of synthetic.synth_atmosphere, Gauss-Legendre weights
as float32 products.  Gases are merged in sequence with rank()'s rebinning, and every main-loop step of every merge
(G * G - G + 1 of them; the peeled tail has its own static bound) records d = the number of other row heads below the
re-entering key.  A pass that ends at the first chunk boundary above every lane's d costs 1 + 2 (c - 1) min / max plus one
compare per boundary tested; the full pass of a 20-entry list costs 38.

Orientation: "a rows" is the kernel without kMergeOrient (rows = the running spectrum a), "larger rows" takes per lane the
operand with the larger top ordinate as the rows (b only where a is non-decreasing).  Groupings: 64 wavenumbers of one layer
(the kernel's wave), 8 wavenumbers x 8 layers and 2 x 32 (lanes regrouped over layers: the follow-up of section 9).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from archnemesis_dist_amd import synthetic as syn   # noqa: E402  (no GPU needed for the synthetic inputs)


def bench_family_k(rng, W, G, S, p_bar, temp):
    """(W, L, S, G): k of every gas at every layer's p, T."""
    u = lambda lo, hi, shape: lo + (hi - lo) * rng.random(shape)
    base = 10.0 ** u(-28, -21, (W, 1, S, 1))
    shape = np.sort(10.0 ** u(-2, 3, (W, 1, S, G)), axis=3)
    pexp, texp = u(0.0, 0.3, (W, 1, S, 1)), u(-1.0, 2.0, (W, 1, S, 1))
    return base * shape * p_bar[None, :, None, None] ** pexp * (temp[None, :, None, None] / 200.0) ** texp


def rebin(vals, w, g_ord):
    """rank(): the sorted (value, weight) sequence of every lane re-binned onto g_ord.  vals, w: (N, G*G) in sorted order."""
    cum = np.cumsum(w, axis=1)
    lo = cum - w
    out = np.empty((vals.shape[0], len(g_ord) - 1))
    for ig in range(len(g_ord) - 1):
        ov = np.clip(np.minimum(cum, g_ord[ig + 1]) - np.maximum(lo, g_ord[ig]), 0.0, None)
        out[:, ig] = (ov * vals).sum(axis=1) / np.maximum(ov.sum(axis=1), 1e-300)
    return out


def entry_depths(rows, cols):
    """d of every main-loop step of every lane: (N, G*G - G + 1).  rows, cols: (N, G), both ascending."""
    N, G = rows.shape
    sums = rows[:, :, None] + cols[:, None, :]
    order = np.argsort(sums.reshape(N, G * G), axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(G * G)[None, :].repeat(N, 0), axis=1)
    rank = np.concatenate([rank.reshape(N, G, G), np.full((N, G, 1), G * G + 1)], axis=2)      # column G: the sentinel
    heads = rank[:, :, 0].copy()
    col = np.zeros((N, G), dtype=np.int64)
    ar = np.arange(N)
    nsteps = G * G - G + 1
    d = np.empty((N, nsteps), dtype=np.int64)
    for t in range(nsteps):
        i = np.argmin(heads, axis=1)
        col[ar, i] += 1
        x = rank[ar, i, col[ar, i]]
        heads[ar, i] = x
        d[:, t] = (heads < x[:, None]).sum(axis=1)          # the other heads below x; a sentinel x: all of them
    return d


def pass_cost(dmax, bounds, G):
    """fp64 instructions of the list pass per step (mean) when it ends at the first boundary above dmax."""
    full = 2 * G - 2
    cost = np.full(dmax.shape, float(full + len(bounds)))
    done = np.zeros(dmax.shape, dtype=bool)
    for n, c in enumerate(bounds):
        hit = ~done & (dmax < c)
        cost[hit] = 1 + 2 * (c - 1) + (n + 1)
        done |= hit
    return cost.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waves", type=int, default=64, help="wavenumbers simulated")
    ap.add_argument("--layers", type=int, default=5, help="layers sampled evenly from the bench atmosphere's 100 (32 for the 2 x 32 grouping)")
    ap.add_argument("--ng", type=int, default=20)
    ap.add_argument("--gases", type=int, default=8)
    ap.add_argument("--seed", type=int, default=20260704)
    args = ap.parse_args()
    W, G, S = args.waves, args.ng, args.gases
    rng = np.random.default_rng(args.seed)
    atm = syn.synth_atmosphere(100, S, seed=7)
    lay = np.linspace(0, 99, args.layers).round().astype(int)
    p_bar, temp, amount = atm["lay_press_pa"][0][lay] / 1e5, atm["lay_temp"][0][lay], atm["amount"][0][:, lay]
    L = len(lay)
    _, delg = syn.gauss_legendre_01(G, as_float32=True)
    dg = delg.astype(np.float32)
    wpair = (dg[:, None] * dg[None, :]).astype(np.float64)
    g_ord = np.concatenate([[0.0], np.cumsum(dg).astype(np.float64)])
    g_ord[G] = 1.0
    tau = bench_family_k(rng, W, G, S, p_bar, temp) * amount.T[None, :, :, None]         # (W, L, S, G)
    N = W * L
    a = tau[:, :, 0].reshape(N, G)
    depth = {"a rows": [], "larger rows": []}
    for s in range(1, S):
        b = tau[:, :, s].reshape(N, G)
        swap = (b[:, -1] > a[:, -1]) & np.all(np.diff(a, axis=1) >= 0.0, axis=1)
        a_sorted = np.sort(a, axis=1)                       # the kernel orders the heads of a non-monotone a (merge_init)
        depth["a rows"].append(entry_depths(a_sorted, b))
        rows = np.where(swap[:, None], b, a_sorted)
        cols = np.where(swap[:, None], a_sorted, b)
        depth["larger rows"].append(entry_depths(rows, cols))
        sums = (a[:, :, None] + b[:, None, :]).reshape(N, G * G)
        order = np.argsort(sums, axis=1, kind="stable")
        a = rebin(np.take_along_axis(sums, order, 1), wpair.reshape(-1)[order], g_ord)
    print(f"bench family: {W} wavenumbers x {L} layers, G = {G}, {S} gases in sequence, {G * G - G + 1} main-loop steps per merge")
    groupings = [("64 wavenumbers x 1 layer", 64, 1), ("8 x 8", 8, 8), ("2 x 32", 2, 32)]
    bound_sets = [(4, 8, 12, 16), (2, 5, 9, 14), (3, 7, 12), (8,), (6, 12), (4, 10)]
    for name, dl in depth.items():
        d = np.stack(dl, axis=0).reshape(S - 1, W, L, -1)    # merge, wavenumber, layer, step
        print(f"\n{name}: mean d per lane {d.mean():.2f}")
        for gname, gw, gl in groupings:
            if W % gw or L % gl:
                print(f"  {gname}: needs --waves a multiple of {gw} and --layers a multiple of {gl}")
                continue
            dm = d.reshape(S - 1, W // gw, gw, L // gl, gl, -1).max(axis=(2, 4))
            costs = ", ".join(f"{'/'.join(map(str, bs))}: {pass_cost(dm, bs, G):.1f}" for bs in bound_sets if bs[-1] < G - 2)
            print(f"  {gname}: mean of the max of d {dm.mean():.1f}, {100.0 * (dm >= G - 1).mean():.0f} % of steps at {G - 1}; "
                  f"fp64 list instructions per step (full pass {2 * G - 2}) with boundaries {costs}")


if __name__ == "__main__":
    main()
