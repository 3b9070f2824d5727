"""Golden fixture for the ILS cases at the chunk and column-block edges of k_ils_conv (tests/tile_edge_cases.py): the
REFERENCE's Measurement_0.lblconv / lblconvg / lblconv_fil / lblconvg_fil, their *_ngeom variants, conv / convg with FWHM < 0
and the integrate_filter family on every case of ils_cases() and on ils_exact_case().  The inputs are rebuilt from their
seeds by the tests; only the results are stored ("<case>/y", "<case>/g").
Build container only.   python oracle/gen_golden_tile_edges.py"""
import os
import sys
import io
import contextlib
import importlib
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from oracle.ref_import import import_reference  # noqa: E402
import tile_edge_cases as tc  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")


def run_reference(M0, c):
    vw, y, d, vc = c["vwave"], c["y"], c["dydx"], c["vconv"]
    nw, nc = vw.size, vc.size
    ng = "_ngeom" if y.ndim == 2 else ""
    g = "g" if d is not None else ""
    data = (nw, vw, y) + (() if d is None else (d,)) + (nc, vc)
    if c["kind"] == "shape":
        r = getattr(M0, "lblconv" + g + ng)(*data, c["ishape"], c["fwhm"])
    elif c["kind"] == "fil":
        r = getattr(M0, "lblconv" + g + "_fil" + ng)(*data, c["nfil"], c["vfil"], c["afil"])
    elif c["kind"] == "integrate":
        r = getattr(M0, "integrate_filter" + g + ng)(*data, c["nfil"], c["vfil"], c["afil"])
    else:                                                     # the k-table methods, a filter per convolution point
        Meas = M0.Measurement_0()
        Meas.NGEOM = 1; Meas.FWHM = -1.0; Meas.NCONV = np.array([nc]); Meas.VCONV = vc[:, None].copy()
        Meas.NFIL = c["nfil"]; Meas.VFIL = c["vfil"]; Meas.AFIL = c["afil"]
        r = Meas.conv(vw, y, IGEOM=0) if d is None else Meas.convg(vw, y, d, IGEOM=0)
    return r if d is not None else (r, None)


def main():
    import_reference()
    M0 = importlib.import_module("archnemesis.Measurement_0")
    cases = dict(tc.ils_cases(), exact=tc.ils_exact_case())
    out = {}
    sink = io.StringIO()                                      # the un-jitted kernels print for every zero weight
    with contextlib.redirect_stdout(sink), np.errstate(all="ignore"):
        for name, c in cases.items():
            yo, go = run_reference(M0, c)
            out[name + "/y"] = np.asarray(yo, float)
            if go is not None:
                out[name + "/g"] = np.asarray(go, float)
    path = os.path.join(OUT, "tile_edges.npz")
    np.savez_compressed(path, **out)
    print({k: (np.shape(v), int(np.isnan(v).sum())) for k, v in out.items()})
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
