"""Mie golden: the REFERENCE's Scatter_0.makephase (module level, Scatter_0.py:1828 -> miescat :1600 -> dmie :1399) on the
cases of tests/mie_cases.py.  Per case every argument, the reference's xscat, xext, thetax, phas and the number of radii
each wavelength integrated over.  The reference does not return that number: it is the restatement's, which is held to the
reference's result to 1e-12 here (a radius more or less moves the sums by 1e-8 and more).  Needs the reference (build
container only).

Per wavelength of an open range the cut-off decision must have margin: n Q_sca / (1e-6 max) farther than 1e-6 from 1 at the
last radius and at the one before, so that no expected count rests on the rounding of a comparison.

    python tools/golden/gen_golden_mie.py      # -> tests/golden/mie.npz
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.ref_import import import_reference  # noqa: E402
import mie_cases as mc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mie.npz")


def main():
    import_reference()
    sc = importlib.import_module("archnemesis.Scatter_0")      # the package attribute of that name is the class
    blob = {}
    for name, d in mc.golden_cases().items():
        xscat, xext, thetax, phas = sc.makephase(d["wavel"].copy(), int(d["iscat"]), d["dsize"].copy(), d["rs"].copy(),
                                                 d["refindx"].copy(), d["theta"].copy())
        det = {}
        got = mc.makephase_np(d["wavel"], d["iscat"], d["dsize"], d["rs"], d["refindx"], d["theta"], return_counts=True,
                              details=det)
        g = dict(xscat=xscat, xext=xext, phas=phas)
        dev = mc.deviations((got[0], got[1], got[3]), g)
        assert max(dev) < 1e-12 and np.array_equal(got[2], thetax), (name, dev)
        assert phas.shape == (d["wavel"].shape[0], mc.nphas_of(d["theta"])) and np.all(phas > 0) and np.all(xext >= xscat)
        counts = got[4]
        if name in mc.OPEN_CASES:
            for w, p in zip(d["wavel"], det["per_wave"]):
                assert p["ratio_end"] < 1 - 1e-6 and p["ratio_before"] > 1 + 1e-6, (name, w, p)
            ratios = " ".join("%.4f/%.4f" % (p["ratio_end"], p["ratio_before"]) for p in det["per_wave"])
        else:
            assert np.all(counts == mc.EXPECTED_RADII[name]), (name, counts)
            ratios = "closed"
        print(f"{name:18s} radii {counts}  cut-off ratios (last/before) {ratios}  restatement deviation {max(dev):.1e}")
        for k in mc.INPUTS:
            blob[f"{name}__{k}"] = np.asarray(d[k])
        blob[f"{name}__xscat"] = xscat; blob[f"{name}__xext"] = xext; blob[f"{name}__thetax"] = thetax
        blob[f"{name}__phas"] = phas; blob[f"{name}__n_radii"] = np.asarray(counts, dtype=np.int32)
    np.savez_compressed(OUT, **blob)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
