"""Henyey-Greenstein fit goldens: the REFERENCE's Scatter_0.subfithgm (Scatter_0.py:1948) on the cases of
tests/hgfit_cases.py -> tests/golden/hgfit.npz.  Per case the inputs (theta, phase), the reference's f, g1, g2, rms and, per
fit, how often it called mrqminl and how many of the calls were accepted (`singular-90`: the inputs only, the reference
raises there, which the script asserts) (counted by a wrapper around the reference's
mrqminl, which subfithgm resolves by global name; the fits of a call are independent, :1980, so each runs on its own).  Needs
the reference (build container only).

Per case the script prints what tests/test_hgfit_host.py records, for (f, g1, g2) and for rms separately:
HGFIT_DEVIATION = max(deviation of the restatement in the kernel's order from the reference, one-ulp sensitivity), the
sensitivity being the deviation of the restatement in the kernel's order from itself with every cos, log and pow result
moved one ulp up, then down.  It asserts HGFIT_DEVIATION <= 1e-8 for every case (the GPU bound, 100 times that, then stays
under the parity bar of 1e-6; a case above it is replaced by another input, not tolerated) and, in the end, that the table
recorded in tests/test_hgfit_host.py is not smaller (after a change of the cases: paste the printed table, run again).  A
file whose arrays would come out as they are is left alone.

    python tools/golden/gen_golden_hgfit.py      # -> tests/golden/hgfit.npz
    python tools/golden/gen_golden_hgfit.py --measure      # the deviations only
"""
import importlib
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.ref_import import import_reference  # noqa: E402
import hgfit_cases as hc  # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN_DIR, "hgfit.npz")
MEASURE_ONLY = "--measure" in sys.argv      # print the deviations only: nothing asserted, nothing written


def run_reference(sc, theta, phase):
    """the reference fit by fit -> f, g1, g2, rms, counts (nfit, 2)"""
    true_fn = sc.mrqminl
    nfit = phase.shape[0]
    out = np.zeros((4, nfit))
    counts = np.zeros((nfit, 2), dtype=np.int32)
    for i in range(nfit):
        seen = []

        def spy(*a):
            r = true_fn(*a)
            seen.append(int(r[3]))
            return r

        sc.mrqminl = spy
        try:
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore", RuntimeWarning)
                res = sc.subfithgm(theta.copy(), phase[i:i + 1].copy())
        finally:
            sc.mrqminl = true_fn
        out[:, i] = [r[0] for r in res]
        counts[i] = (len(seen), sum(seen))
    return out[0], out[1], out[2], out[3], counts


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
    import_reference()
    sc = importlib.import_module("archnemesis.Scatter_0")
    blob, table, measured = {}, [], {}
    for name, (theta, phase) in hc.cases(GOLDEN_DIR).items():
        ref = run_reference(sc, theta, phase)
        got_ref = hc.subfithgm_np(theta, phase, order="reference", return_counts=True)
        got_ker = hc.subfithgm_np(theta, phase, order="kernel", return_counts=True)
        dev_ref, dev_ker = hc.deviations(got_ref, ref), hc.deviations(got_ker, ref)
        sens = (0.0, 0.0)
        for direction in (1.0, -1.0):
            moved = hc.subfithgm_np(theta, phase, order="kernel", fn=hc.shifted_funcs(direction))
            sens = tuple(max(a, b) for a, b in zip(sens, hc.deviations(moved, got_ker)))
        dev = tuple(max(a, b) for a, b in zip(dev_ker, sens))
        c = ref[4]
        print(f"{name:12s} fits {phase.shape[0]:3d} x {phase.shape[1]:3d} angles  reference calls {c[:, 0].min()} .. {c[:, 0].max()}"
              f" accepted {c[:, 1].min()} .. {c[:, 1].max()}  kernel-order calls {got_ker[4][:, 0].min()} .. {got_ker[4][:, 0].max()}\n"
              f"    reference order %.2e %.2e (counts equal: %s)  kernel order %.2e %.2e  one ulp %.2e %.2e"
              % (dev_ref + (np.array_equal(got_ref[4], c),) + dev_ker + sens), flush=True)
        assert MEASURE_ONLY or all(d <= 1e-8 for d in dev), (name, dev)      # so that 100 x stays under the parity bar's cap of 1e-6
        measured[name] = dev
        table.append('    "%s": (%.2e, %.2e),' % ((name,) + tuple(1.005 * d for d in dev)))      # never rounded down
        blob[f"{name}__theta"] = theta; blob[f"{name}__phase"] = phase
        for k, v in zip(("f", "g1", "g2", "rms", "counts"), ref):
            blob[f"{name}__{k}"] = v
    # the fit the reference cannot do: its own failure is the expected result
    theta, phase = hc.singular_case(GOLDEN_DIR)
    try:
        run_reference(sc, theta, phase)
        raise AssertionError("singular-90: the reference did not fail")
    except np.linalg.LinAlgError as exc:
        print("singular-90  the reference raises LinAlgError: %s" % exc)
    blob["singular-90__theta"] = theta; blob["singular-90__phase"] = phase
    if MEASURE_ONLY:
        return
    write(OUT, blob)
    print("HGFIT_DEVIATION = {\n" + "\n".join(table) + "\n}")
    from test_hgfit_host import HGFIT_DEVIATION          # the record the GPU bounds come from: it must cover what was measured
    stale = [name for name, dev in measured.items() if not all(d <= r for d, r in zip(dev, HGFIT_DEVIATION.get(name, (0, 0))))]
    print("tests/test_hgfit_host.py::HGFIT_DEVIATION " + ("covers every case" if not stale else "is too small for %s" % stale))
    assert not stale


if __name__ == "__main__":
    main()
