"""Pseudo-continuum golden: the REFERENCE's LineData_0.add_pseudo_continuum_monochromatic_absorption (LineData_0.py:486) on the
seeded synthetic bin sets of tests/lbl_pc_cases.py -- six bin geometries with the Voigt shape (regular, jittered with gaps and
overlaps, overlapping, ending inside the grid, starting inside it, more bins than the first touched grid index), a Lorentz
and a Gaussian case, one neighbour bin, a non-zero `out`, two and three broadeners.  Per case the inputs and the reference's
out, store (rows 0 .. 2) and store_x.  Needs the reference (build container only).

    python tools/golden/gen_golden_lbl_pc.py      # -> tests/golden/lbl_pseudo_continuum.npz
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.ref_import import import_reference  # noqa: E402
import lbl_pc_cases as pc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lbl_pseudo_continuum.npz")


def main():
    import_reference()
    ld = importlib.import_module("archnemesis.LineData_0")      # the package attribute of that name is the class
    ls = importlib.import_module("archnemesis.lineshape")
    fns = {pc.VOIGT: ls.voigt, pc.LORENTZ: ls.lorentz, pc.GAUSSIAN: ls.gaussian}
    blob = {}
    for name, d in pc.golden_cases().items():
        N, nb = d["centers"].shape[0], d["n_neighbour_bins"]
        shape_fn = fns[d["lineshape_id"]]
        smallest = [np.inf]

        def watched(dwn, alpha_d, gamma_l, _f=shape_fn, _s=smallest):
            v = _f(dwn, alpha_d, gamma_l)
            if v != 0.0:
                _s[0] = min(_s[0], float(v))
            return v

        out = d["out0"].copy()
        store, store_x = np.zeros((3, N)), np.zeros(N)
        ld.add_pseudo_continuum_monochromatic_absorption(
            d["wn_grid"], watched, d["t_calc"], d["t_ref"], d["p_calc"], d["p_ref"], d["q_ratio"], d["isotopic_abundance"],
            d["isotopic_mass"], d["mol_mix_frac"], d["bparams"], d["centers"], d["widths"], d["sw_sum"], d["e_lower"], out,
            store=store, store_x=store_x, n_neighbour_bins=nb)
        # no expected value rests on subnormal arithmetic
        assert smallest[0] >= 1e-280, (name, smallest[0])
        nz = int(np.count_nonzero(out - d["out0"]))
        print(f"{name:18s} N={N:4d} shape={pc.SHAPE_NAMES[d['lineshape_id']]:8s} nb={nb}  changed grid points {nz:4d} of "
              f"{out.size}  smallest shape {smallest[0]:.2e}")
        assert (nz >= out.size - 1) == (name in pc.COVERING), name
        for k in pc.INPUTS:
            blob[f"{name}__{k}"] = np.asarray(d[k])
        blob[f"{name}__out"] = out; blob[f"{name}__store"] = store; blob[f"{name}__store_x"] = store_x
    np.savez_compressed(OUT, **blob)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
