#!/usr/bin/env python
"""C4-LBL timing: CIRSrad's multiple-scattering branch on an LBL table (2e5 nu x G 1 x 100 layers, haze + Rayleigh) with the
G = 1 spectral windows against one window over the whole axis (ANSFM_MS_WINDOW = W), at 16 streams / NF 8 and 5 streams /
NF 2.  Device-synchronised wall time (the entry point returns after its copy back) after one warm-up call per setting.

    python3 tools/c4_lbl_run.py [W] [reps]                     # prints one JSON line per setting
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_c4_lbl -o run -- python3 tools/c4_lbl_run.py 200000 1
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import archnemesis_dist_amd as pkg  # noqa: E402
from archnemesis_dist_amd import synthetic as syn  # noqa: E402

W = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
S, L, NP, NT = 2, 100, 6, 4

eng = pkg.AnsfmEngine(0)
rng = np.random.default_rng(3)
PRESS = np.logspace(-5, 1, NP); TEMP = np.linspace(90.0, 300.0, NT)
K = (10.0 ** rng.uniform(-25, -21, (W, 1, 1, S))) * PRESS[None, :, None, None] ** 0.15 * (TEMP[None, None, :, None] / 150.0) ** 0.8
WAVE = 200.0 + 0.01 * np.arange(W)
eng.upload_lbltable(K, PRESS, TEMP, WAVE); del K
atm = syn.synth_atmosphere(L, S, seed=7)
lay_p, lay_t, am = atm["lay_press_pa"][0], atm["lay_temp"][0], atm["amount"][0]
TH = np.linspace(0.0, 180.0, 41); c = np.cos(np.deg2rad(TH))
leg = np.polynomial.legendre.legval(c, 0.6 ** np.arange(36) * (2 * np.arange(36) + 1)) / (4 * np.pi)
ph = np.zeros((1, W, 2, TH.size)); ph[0, :, 0, :] = leg[None, :]; ph[0, :, 1, :] = c[None, :]
ph = np.ascontiguousarray(ph[:, :, :, ::-1])
wv = np.linspace(0, 1, W)[:, None]; lv = np.linspace(0, 1, L)[None, :]
TAURAY = 1e-3 * np.exp(-5.0 * lv) * (1.0 + 0.3 * wv)
TAUSCAT = 2e-2 * np.exp(-((lv - 0.35) / 0.1) ** 2) * (1.0 + 0.5 * np.sin(7.0 * wv))
lfrac = np.ones((W, 1, L))


def run(nmu, nf):
    x, w = np.polynomial.legendre.leggauss(nmu)
    MU, WT = 0.5 * (x + 1.0), 0.5 * w
    radg = np.repeat((1.1911e-12 * WAVE ** 3 / (np.exp(1.439 * WAVE / lay_t[0]) - 1.0))[:, None], nmu, 1)
    brdf = np.zeros((W, nmu, nmu, nf + 1))
    return lambda: eng.cirsrad_ck_scatter(0, lay_p, lay_t, am, None, 1.1 * TAUSCAT, TAURAY, TAUSCAT, ph, lfrac, radg, [30.0], [20.0],
                                          [45.0], np.full(W, 1e-8), 0, brdf, MU, WT, nf, 101, 1, 1)


for nmu, nf in ((16, 8), (5, 2)):
    f = run(nmu, nf)
    res = {}
    for tag, win in (("windowed", None), ("one_window", str(W))):
        if win is None:
            os.environ.pop("ANSFM_MS_WINDOW", None)
        else:
            os.environ["ANSFM_MS_WINDOW"] = win
        out = f()                                                   # warm-up (and buffers)
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter(); out2 = f(); ts.append(time.perf_counter() - t0)
        nw, ww = eng.last_scatter_windows()
        res[tag] = dict(wall_s=min(ts), windows=nw, window_wavenumbers=ww, same_bits=bool(np.array_equal(out, out2)))
        res[tag + "_spectrum"] = out2
    os.environ.pop("ANSFM_MS_WINDOW", None)
    same = bool(np.array_equal(res.pop("windowed_spectrum"), res.pop("one_window_spectrum")))
    print(json.dumps(dict(config="c4_lbl", W=W, L=L, nmu=nmu, nf=nf, windowed_equals_one_window=same, **res)), flush=True)
eng.close()
