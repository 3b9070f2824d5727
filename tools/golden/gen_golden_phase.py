"""Phase-function golden: the REFERENCE's Scatter_0.calc_phase (Scatter_0.py:760) for IMIE 0 / 1 / 2 and calc_phase_ray (:834)
on the cases of tests/phase_cases.py.  Needs the reference (build container only); never run by a test.

Per case: every input, `ref` (the reference's result) and `ulp` -- the largest change of the NumPy restatement, relative to the
column maximum over the angles, when the result of every cos and pow is moved by one np.nextafter (all up, all down, and
alternating from call site to call site both ways).  The GPU tests allow 16 times that figure for the modes that have a cos or
a pow; the tabulated mode has neither and is compared bit for bit.  Asserted here: the restatement gives the reference's bits
for the tabulated mode and is within 4 x ulp of it elsewhere, and 16 x ulp <= 1e-6, the project's parity bar.

    python tools/golden/gen_golden_phase.py      # -> tests/golden/phase.npz
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.ref_import import import_reference  # noqa: E402
import phase_cases as pc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "phase.npz")


def scatter_of(sc, d):
    """a Scatter_0 that holds the case's tables"""
    imie, tab = int(d["imie"]), d["tab"]
    s = sc.Scatter_0(IMIE=imie, NDUST=tab.shape[2])
    s.NWAVE = d["swave"].shape[0]
    s.WAVE = d["swave"].copy()
    if imie == 0:
        s.F, s.G1, s.G2 = tab[0].copy(), tab[1].copy(), tab[2].copy()
    elif imie == 1:
        s.NTHETA = d["ttab"].shape[0]
        s.THETA = d["ttab"].copy()
        s.PHASE = tab.copy()
    else:
        s.NLPOL = tab.shape[1]
        s.WLPOL = tab.copy()
    return s


def main():
    import_reference()
    sc = importlib.import_module("archnemesis.Scatter_0")
    blob = {}
    for name, d in pc.golden_cases().items():
        if "imie" in d:
            ref = scatter_of(sc, d).calc_phase(d["theta"].copy(), d["wave"].copy())
            assert ref.shape == (d["wave"].shape[0], d["theta"].shape[0], d["tab"].shape[2])
        else:
            ref = sc.Scatter_0().calc_phase_ray(d["theta"].copy())
        got = pc.evaluate_np(d)
        dev = pc.deviation(got, ref)
        ulp = max(pc.deviation(pc.evaluate_np(d, pc.Nudge(p)), got) for p in pc.PATTERNS)
        print(f"{name:10s} restatement {dev:.1e}   one ulp {ulp:.1e}   GPU bound {16 * ulp:.1e}")
        if int(d.get("imie", -1)) in pc.EXACT_KINDS:
            assert np.array_equal(got, ref), name
            assert ulp == 0.0
        else:
            assert dev <= 4 * ulp, (name, dev, ulp)
        assert 16 * ulp <= 1e-6, (name, ulp)
        for k, v in d.items():
            blob[f"{name}__{k}"] = np.asarray(v)
        blob[f"{name}__ref"] = ref
        blob[f"{name}__ulp"] = np.asarray(ulp)
        if int(d.get("imie", -1)) == 0:      # the slots of the scattering array, np.interp as ForwardModel_0.py:5131-5133 calls it
            blob[f"{name}__hg"] = pc.hg_on_grid(d["swave"], d["tab"], d["wave"])
    np.savez_compressed(OUT, **blob)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
