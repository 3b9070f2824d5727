#!/usr/bin/env python
"""CIRSrad on runtime line-by-line opacities (ILBL = 1) without the reference: a synthetic gas of three isotopologues goes
into HBM once as a line source; a state -- here a nadir column and three perturbed copies, as a numerical Jacobian makes
them -- is packed into its distinct k-rows, and the thermal-emission call takes its gas opacities from the lines.

    python examples/c5_cirsrad.py [points] [layers]     # needs an MI355X and a built libansfm.so
"""
import os
import sys
import time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import archnemesis_dist_amd as pkg                                    # noqa: E402
from archnemesis_dist_amd import line_source as ls                     # noqa: E402
from archnemesis_dist_amd import synthetic as syn                      # noqa: E402


def main():
    nw = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    eng = pkg.AnsfmEngine(0)
    wn = 2000.0 + 1e-3 * np.arange(nw)
    src = syn.synth_line_source(wn, (3,), max(nw // 10, 100), seed=3)
    t0 = time.perf_counter(); eng.upload_line_source(src); t_up = time.perf_counter() - t0     # lines sorted and uploaded once
    lp = 101325.0 * np.logspace(0, -4, L); lt = np.linspace(300.0, 150.0, L)
    am = 1.0e22 * (lp / lp[0])[None, :]
    mix = np.array([[0.05, 0.95]])                                     # (self, ambient) of the gas: 1 - amb_frac, amb_frac
    NLAYIN, LAYINC, SCALE = syn.nadir_path(L, 10.0)
    cont = np.zeros((nw, L))

    # one state
    t0 = time.perf_counter()
    eng.set_line_state(ls.pack_line_state(src, lp / ls.ATM_TO_PASCAL, lt, mix))
    spec = eng.cirsrad_ck_thermal(0, lp, lt, am, cont, NLAYIN, LAYINC, SCALE, lt[LAYINC[:, 0]][:, None], -1.0)
    t1 = time.perf_counter() - t0
    taugas = eng.get_taugas(L, 0)
    print(f"{nw} points x {L} layers, {src.n_iso[0]} isotopologues x {src.gases[0][0].N} lines: upload {t_up * 1e3:.1f} ms, "
          f"state + CIRSrad {t1 * 1e3:.1f} ms; rows {eng.last_line_rows()[0]}")
    print("  radiance:", spec[:3, 0], " column opacity range:", float(taugas.sum(axis=2).min()), float(taugas.sum(axis=2).max()))

    # four states of a Jacobian: state 0, a layer temperature, the gas scaled (its mix fractions change), a copy of state 0
    n = 4
    LP, LT, AM, MIX = (np.repeat(a[None], n, 0) for a in (lp, lt, am, mix))
    LT[1, L // 2] += 1.0
    AM[2] *= 1.05; MIX[2, 0] = [0.0525, 0.9475]
    st = ls.pack_line_state(src, LP / ls.ATM_TO_PASCAL, LT, MIX)
    t0 = time.perf_counter()
    eng.set_line_state(st)
    specs = eng.cirsrad_ck_thermal(0, LP, LT, AM, np.repeat(cont[None], n, 0), NLAYIN, LAYINC, np.repeat(SCALE[None], n, 0),
                                   np.stack([t[LAYINC[:, 0]][:, None] for t in LT]), np.full(n, -1.0))
    t4 = time.perf_counter() - t0
    print(f"  {n} states: {st.R} distinct rows of {n * L} (model, layer) pairs, {t4 * 1e3:.1f} ms; state 3 equals state 0: "
          f"{bool(np.array_equal(specs[3], specs[0]))}, state 0 equals the single call: {bool(np.array_equal(specs[0], spec))}")
    eng.close()


if __name__ == "__main__":
    main()
