"""Mie goldens: the REFERENCE's Scatter_0.makephase (module level, Scatter_0.py:1828 -> miescat :1600 -> dmie :1399) on the
cases of tests/mie_cases.py: golden_cases() -> tests/golden/mie.npz, edge_cases() -> tests/golden/mie_edges.npz.  Per case
every argument, the reference's xscat, xext, thetax, phas and the number of radii each wavelength integrated over.  The
reference does not return that number: it is the restatement's, which is held to the reference's result to 1e-12 here (a
radius more or less moves the sums by 1e-8 and more).  Needs the reference (build container only).

Per wavelength of an open range the cut-off decision must have margin: n Q_sca / (1e-6 max) farther than 1e-6 from 1 at the
last radius and at the one before, so that no expected count rests on the rounding of a comparison.

The reference treats the wavelengths of a call one after the other and independently (:1905), so the edge cases, two of
which take the un-jitted reference minutes, are run one wavelength per task on a pool of processes.  For every edge case
the script also prints what tests/test_mie_host.py records: the restatement's deviation in both orders of the sum, and
EDGE_DEVIATION = max(chunk-order deviation, one-ulp sensitivity), and in the end asserts that the table recorded there is
not smaller (after a change of the cases: paste the printed table, run again).  A file whose arrays would come out as they are is left
alone (the archive's time stamps would change its bytes).

    python tools/golden/gen_golden_mie.py      # -> tests/golden/mie.npz, tests/golden/mie_edges.npz
"""
import importlib
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.ref_import import import_reference  # noqa: E402
import mie_cases as mc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mie.npz")
OUT_EDGES = os.path.join(ROOT, "tests", "golden", "mie_edges.npz")
_sc = None


def reference():
    global _sc
    if _sc is None:
        import_reference()
        _sc = importlib.import_module("archnemesis.Scatter_0")      # the package attribute of that name is the class
    return _sc


def run_reference(d, waves=slice(None)):
    return reference().makephase(d["wavel"][waves].copy(), int(d["iscat"]), d["dsize"].copy(), d["rs"].copy(),
                                 d["refindx"][waves].copy(), d["theta"].copy())


def _one_wavelength(task):
    name, i = task
    return name, i, run_reference(mc.edge_cases()[name], slice(i, i + 1))


def reference_by_wavelength(cases):
    """name -> (xscat, xext, thetax, phas), every wavelength a task of its own, the longest first"""
    tasks = [(name, i) for name, d in cases.items() for i in range(d["wavel"].shape[0])]
    cost = lambda t: -(mc.radius_count(cases[t[0]]["rs"]) or 200) * cases[t[0]]["rs"][0] / cases[t[0]]["wavel"][t[1]]
    tasks.sort(key=cost)
    out = {name: [None] * d["wavel"].shape[0] for name, d in cases.items()}
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        for name, i, res in pool.imap_unordered(_one_wavelength, tasks):
            out[name][i] = res
    joined = {}
    for name, rows in out.items():
        assert all(np.array_equal(r[2], rows[0][2]) for r in rows), name
        joined[name] = (np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]), rows[0][2],
                        np.concatenate([r[3] for r in rows], axis=0))
    return joined


def check_case(name, d, ref, open_cases, expected):
    """the assertions on one case; returns its arrays for the file and the restatement's deviation"""
    xscat, xext, thetax, phas = ref
    det = {}
    got = mc.makephase_np(d["wavel"], d["iscat"], d["dsize"], d["rs"], d["refindx"], d["theta"], return_counts=True,
                          details=det)
    g = dict(xscat=xscat, xext=xext, phas=phas)
    dev = mc.deviations((got[0], got[1], got[3]), g)
    assert max(dev) < 1e-12 and np.array_equal(got[2], thetax), (name, dev)
    assert phas.shape == (d["wavel"].shape[0], mc.nphas_of(d["theta"])) and np.all(phas > 0) and np.all(xext >= xscat)
    counts = got[4]
    if name in open_cases:
        for w, p in zip(d["wavel"], det["per_wave"]):
            assert p["ratio_end"] < 1 - 1e-6 and p["ratio_before"] > 1 + 1e-6, (name, w, p)
        ratios = " ".join("%.4f/%.4f" % (p["ratio_end"], p["ratio_before"]) for p in det["per_wave"])
    else:
        ratios = "closed"
    if name in expected:
        assert np.all(counts == expected[name]), (name, counts)
    print(f"{name:18s} radii {counts if counts.shape[0] <= 4 else '%d x %d' % (counts.shape[0], counts[0])}  "
          f"cut-off ratios (last/before) {ratios}  restatement deviation {max(dev):.1e}", flush=True)
    blob = {f"{name}__{k}": np.asarray(d[k]) for k in mc.INPUTS}
    blob[f"{name}__xscat"] = xscat; blob[f"{name}__xext"] = xext; blob[f"{name}__thetax"] = thetax
    blob[f"{name}__phas"] = phas; blob[f"{name}__n_radii"] = np.asarray(counts, dtype=np.int32)
    return blob, g, dev


def write(path, blob):
    if os.path.exists(path):
        old = np.load(path)
        same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        if list(old.files) == list(blob) and all(same(old[k], np.asarray(v)) for k, v in blob.items()):
            print("unchanged", path, os.path.getsize(path), "bytes")
            return
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes")


def main():
    blob = {}
    for name, d in mc.golden_cases().items():
        blob.update(check_case(name, d, run_reference(d), mc.OPEN_CASES, mc.EXPECTED_RADII)[0])
    write(OUT, blob)

    cases = mc.edge_cases()
    assert set(mc.EDGE_EXPECTED_RADII) == set(cases) and not set(cases) & set(mc.golden_cases())
    refs = reference_by_wavelength(cases)
    blob, table, measured = {}, [], {}
    for name, d in cases.items():
        b, g, dev = check_case(name, d, refs[name], mc.EDGE_OPEN_CASES, mc.EDGE_EXPECTED_RADII)
        blob.update(b)
        chunk = mc.makephase_np(d["wavel"], d["iscat"], d["dsize"], d["rs"], d["refindx"], d["theta"], chunk_order=True)
        dev_chunk = mc.deviations((chunk[0], chunk[1], chunk[3]), g)
        sens = mc.one_ulp_sensitivity(d)
        edge = tuple(max(a, b) for a, b in zip(dev_chunk, sens))
        assert all(100.0 * e <= 1e-6 for e in edge), (name, edge)       # the GPU bound must not need the cap lifted
        print("    reference order %.2e %.2e %.2e  chunk order %.2e %.2e %.2e  one ulp %.2e %.2e %.2e" % (dev + dev_chunk + sens),
              flush=True)
        measured[name] = edge
        table.append('    "%s": (%.2e, %.2e, %.2e),' % ((name,) + tuple(1.005 * e for e in edge)))     # never rounded down
        table.append("        # restatement pointwise, the larger of the two orders: %.2e" % max(dev[2], dev_chunk[2]))
    write(OUT_EDGES, blob)
    print("EDGE_DEVIATION = {\n" + "\n".join(table) + "\n}")
    from test_mie_host import EDGE_DEVIATION          # the record the GPU bounds come from: it must cover what was measured
    stale = [name for name, edge in measured.items() if not all(e <= r for e, r in zip(edge, EDGE_DEVIATION.get(name, (0, 0, 0))))]
    print("tests/test_mie_host.py::EDGE_DEVIATION " + ("covers every case" if not stale else "is too small for %s" % stale))
    assert not stale


if __name__ == "__main__":
    main()
