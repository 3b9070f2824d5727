"""How far the CPU oracle itself is from exact arithmetic on the ill-conditioned case that tests/test_merge_layer_groups.py
prints and does not assert: the boxed k-table of _sweep_k kinds with float64 weights at W = 70, L = 1 (CPU only, no GPU).

  python tools/experiments/r08_oracle_conditioning_probe.py [G = 20] [wavenumber = 38]

For one wavenumber it repeats the reference's sequence of merges (skip rules, sums a_i + b_j as rounded doubles, weights
del_g[i] * del_g[j] as rounded doubles, g_ord as the reference's float cumsum) with the rebinning itself -- cumulative
weights, the overlap of every element with every bin, the division by the bin width -- in rational arithmetic, rounding to
double once per merge, and prints it beside the oracle's gas opacities.  At G = 20, wavenumber 38 the bins 7 and 8 (0.59 and
1.51, just below a jump to 1.3e5) differ by 1.7e-10 and 3.3e-10 relative; every other bin agrees to 1e-13 or better.
"""
import os
import sys
from fractions import Fraction as F

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as orc                    # noqa: E402
import test_merge_layer_groups as T                 # noqa: E402  (the test's own case generator)


def rank_exact(vals, wts, g_ord, G):
    order = sorted(range(len(vals)), key=lambda i: (vals[i], i))
    out = [F(0)] * G
    cum = F(0)
    for i in order:
        lo, cum = cum, cum + wts[i]
        for b in range(G):
            ov = min(cum, g_ord[b + 1]) - max(lo, g_ord[b])
            if ov > 0:
                out[b] += ov * vals[i]
    return [out[b] / (g_ord[b + 1] - g_ord[b]) for b in range(G)]


def main():
    G = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    w0 = int(sys.argv[2]) if len(sys.argv) > 2 else 38
    orc.build()
    rng = np.random.default_rng(9000 + G)           # test_cirsrad_layer_groups: the first case it draws
    W, L = T.SHAPES[0]
    c = T._cirsrad_case(rng, W, G, 3, L, False, False)
    a = c["atm"]
    _, rtg = orc.cirsrad_ck_thermal(0, c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"], a["lay_press_pa"][0],
                                    a["lay_temp"][0], a["amount"][0], c["cont"][0], c["NLAYIN"], c["LAYINC"], c["SCALE"],
                                    c["EMTEMP"], -1.0, return_taugas=True)
    k = orc.calc_k(c["K"], c["PRESS"], c["TEMP"], a["lay_press_pa"][0] / 101325.0, a["lay_temp"][0])
    am = a["amount"][0]
    assert np.array_equal(orc.k_overlap(c["delg"], k, am * 1.0), rtg)      # the fused oracle = calc_k, then k_overlap
    dg = [F(float(x)) for x in c["delg"]]
    g_ord, acc = [F(0)], 0.0
    for x in c["delg"]:
        acc += float(x)
        g_ord.append(F(acc))
    g_ord[G] = F(1)
    l0 = 0
    tau = [F(float(k[w0, g, l0, 0]) * float(am[0, l0])) for g in range(G)]
    for s in range(1, am.shape[0]):
        b = [F(float(k[w0, g, l0, s]) * float(am[s, l0])) for g in range(G)]
        if b[-1] <= 0:
            continue
        if tau[-1] <= 0:
            tau = b
            continue
        vals = [F(float(tau[i] + b[j])) for i in range(G) for j in range(G)]
        wts = [F(float(dg[i] * dg[j])) for i in range(G) for j in range(G)]
        tau = [F(float(x)) for x in rank_exact(vals, wts, g_ord, G)]
    print(f"G = {G}, wavenumber {w0}, layer {l0}:  bin, exact rebinning, oracle, (oracle - exact) / exact")
    for g in range(G):
        e, o = float(tau[g]), float(rtg[w0, g, l0])
        print(f"{g:3d} {e!r:>24} {o!r:>24} {(o - e) / e if e else 0.0: .3e}")


if __name__ == "__main__":
    main()
