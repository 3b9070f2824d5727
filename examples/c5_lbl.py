#!/usr/bin/env python
"""Runtime line-by-line opacity without the reference: a synthetic gas of two isotopologues -- per isotopologue the lines
(LineData_0.add_line_set_monochromatic_absorption) and the pseudo-continuum of the weak lines
(add_pseudo_continuum_monochromatic_absorption), the two sums of calculate_monochromatic_absorption -- summed in HBM by the
engine's accumulator and read back once, beside the same four calls on a host array.

    python examples/c5_lbl.py [points] [layers]     # needs an MI355X and a built libansfm.so
"""
import os
import sys
import time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import archnemesis_dist_amd as pkg                                    # noqa: E402
from archnemesis_dist_amd import synthetic as syn                      # noqa: E402


def main():
    nw = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    eng = pkg.AnsfmEngine(0)
    wn = 2000.0 + 1e-3 * np.arange(nw)
    t, p = np.linspace(150.0, 300.0, L), np.logspace(-4, 0, L)
    gas = syn.synth_lbl_gas(wn[0], wn[-1], 2, max(nw // 10, 100), L, seed=3)

    def through_accumulator():
        acc = eng.lbl_accumulator(wn, t, p)               # grid and (T, p) go up once; a zeroed (L, nw) in HBM
        for lines, cont in gas:
            acc.add_lines(*lines)
            acc.add_pseudo_continuum(*cont)
        return acc

    def through_host_arrays():
        k = np.zeros((L, nw))
        for lines, cont in gas:
            eng.add_line_set_monochromatic_absorption(wn, lines[0], t, lines[1], p, *lines[2:], k)
            eng.add_pseudo_continuum_monochromatic_absorption(wn, cont[0], t, cont[1], p, *cont[2:], k)
        return k

    through_accumulator(); through_host_arrays()
    t0 = time.perf_counter(); k_acc = through_accumulator().numpy(); ta = time.perf_counter() - t0
    t0 = time.perf_counter(); k_host = through_host_arrays(); th = time.perf_counter() - t0
    cont_only = np.zeros((L, nw))
    for _, cont in gas:
        eng.add_pseudo_continuum_monochromatic_absorption(wn, cont[0], t, cont[1], p, *cont[2:], cont_only)
    print(f"{nw} points x {L} layers, 2 isotopologues ({gas[0][0][8].size} lines, {gas[0][1][8].size} bins each)")
    print(f"  accumulator {ta * 1e3:8.1f} ms   four host-array calls {th * 1e3:8.1f} ms   same bits: {bool(np.array_equal(k_acc, k_host))}")
    print("  k [cm2 / molecule], first layer:", k_acc[0, :3], " pseudo-continuum share at the median point:",
          float(np.median(cont_only[0, :-1] / k_acc[0, :-1])))
    dev = through_accumulator().torch()                   # ... or stays in HBM for a next step
    print("  as a torch tensor:", tuple(dev.shape), dev.device, float(dev.sum()))


if __name__ == "__main__":
    main()
