"""Surface-reflection golden: the REFERENCE's calc_Hapke_BRDF (Surface_0.py:1292), calc_OrenNayar_BRDF (:1743),
Surface_0.calc_BRDF (:916) for LOWBC 1 / 2 / 3 and ForwardModel_0.calc_brdf_matrix (ForwardModel_0.py:5168) on the cases of
tests/brdf_cases.py.  Needs the reference (build container only).

Per case: every input, the reference's result, and `ulp` -- the largest deviation from the reference, relative to the row
(matrix: plane) maximum, of the NumPy restatement re-evaluated with cg and the result of every cos / sin / tan / exp / log /
arccos / sqrt / pow moved by one np.nextafter (all up, all down, and alternating from call site to call site both ways).
The GPU tests allow 16 times that figure: the dozen chained device functions may each err by a few ulp, not one, and need
not share a sign.  Asserted here: the restatement itself is within 1e-13 of the reference, and 16 x ulp <= 1e-6, the
project's parity bar -- a case that misses it gets other inputs, not another bar.

    python tools/golden/gen_golden_brdf.py      # -> tests/golden/brdf.npz
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.ref_import import import_reference  # noqa: E402
import brdf_cases as bc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "brdf.npz")


def surface_of(su, lowbc, params, wave):
    """a Surface_0 whose interpolation onto `wave` returns the case's parameters: the spectral grid is the case's own"""
    s = su.Surface_0(GASGIANT=False, LOWBC=lowbc, GALB=-1.0, NEM=wave.shape[0])
    s.VEM = wave.copy()
    if lowbc == 1:
        s.EMISSIVITY = 1.0 - params[0]
        assert np.array_equal(1.0 - s.EMISSIVITY, params[0])      # calc_albedo's 1 - emissivity gives the case's albedo back
    elif lowbc == 2:
        for name, row in zip(("SGLALB", "K", "BS0", "hs", "BC0", "hc", "ROUGHNESS", "G1", "G2", "F"), params):
            setattr(s, name, row.copy())
    else:
        s.ALBEDO = params[0].copy(); s.ROUGHNESS = params[1].copy()
    return s


def main():
    import_reference()
    su = importlib.import_module("archnemesis.Surface_0")
    fm = importlib.import_module("archnemesis.ForwardModel_0")
    blob = {}
    for name, d in bc.golden_cases().items():
        lowbc, P = int(d["lowbc"]), d["params"]
        wave = 1000.0 + 10.0 * np.arange(P.shape[1])
        surf = surface_of(su, lowbc, P, wave)
        if d["kind"] == "points":
            ref = surf.calc_BRDF(wave, d["sol"].copy(), d["emi"].copy(), d["azi"].copy())
            if lowbc == 2:      # the module-level functions give what the class method gives
                assert np.array_equal(ref, su.calc_Hapke_BRDF(*[r.copy() for r in P], d["sol"], d["emi"], d["azi"]))
            elif lowbc == 3:
                assert np.array_equal(ref, su.calc_OrenNayar_BRDF(P[0].copy(), P[1].copy(), d["sol"], d["emi"], d["azi"]))
            assert ref.shape == (P.shape[1], d["sol"].shape[0])
        else:
            scat = types.SimpleNamespace(NMU=len(d["MU"]), MU=d["MU"].copy(), NPHI=int(d["NPHI"]), NF=int(d["NF"]))
            ref = fm.ForwardModel_0.calc_brdf_matrix(None, WAVEC=wave, Scatter=scat, Surface=surf)
            assert ref.shape == (P.shape[1], scat.NMU, scat.NMU, scat.NF + 1)
        dev = bc.deviation(bc.evaluate_np(d), ref)
        ulp = max(bc.deviation(bc.evaluate_np(d, bc.Nudge(p)), ref) for p in bc.PATTERNS)
        print(f"{name:18s} restatement {dev:.1e}   one ulp {ulp:.1e}   GPU bound {16 * ulp:.1e}")
        assert dev <= 1e-13, (name, dev)
        assert 16 * ulp <= 1e-6, (name, ulp)
        blob[f"{name}__kind"] = np.asarray(d["kind"])
        for k in bc.INPUTS[d["kind"]]:
            blob[f"{name}__{k}"] = np.asarray(d[k])
        blob[f"{name}__ref"] = ref
        blob[f"{name}__ulp"] = np.asarray(ulp)
    np.savez_compressed(OUT, **blob)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
