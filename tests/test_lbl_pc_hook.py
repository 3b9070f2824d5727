"""install_gpu_pseudo_continuum against the REAL reference module (build container only): a call with a built line shape
lands on the engine -- here a test double answered by the NumPy restatement, so the argument mapping is checked against the
reference's own result -- and every case outside the GPU path goes to the reference's function, is counted in DELEGATED and
raises under set_strict(True).  The kernels behind the engine method are covered on the GPU by tests/test_lbl_pc_gpu.py."""
import importlib
import os
import sys
import warnings

import numpy as np
import pytest

import lbl_pc_cases as pc

REF = "/root/reference"
pytestmark = [pytest.mark.needs_reference,
              pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "archnemesis")), reason="reference tree not present")]


class EngineDouble:
    def __init__(self):
        self.calls = 0

    def add_pseudo_continuum_monochromatic_absorption(self, wn_grid, lineshape_id, t_calc, t_ref, p_calc, p_ref, q_ratio,
                                                      isotopic_abundance, isotopic_mass, mol_mix_frac, bparams, centers,
                                                      widths, sw_sum, e_lower, out, store=None, store_x=None,
                                                      n_neighbour_bins=3):
        self.calls += 1
        st, x = pc.pseudo_continuum_np(wn_grid, lineshape_id, t_calc, t_ref, p_calc, p_ref, q_ratio, isotopic_abundance,
                                       isotopic_mass, mol_mix_frac, bparams, centers, widths, sw_sum, e_lower, out,
                                       n_neighbour_bins=n_neighbour_bins)
        if store is not None:
            store[...] = st
        if store_x is not None:
            store_x[...] = x
        return out


@pytest.fixture()
def hooked(monkeypatch):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.ref_import import import_reference
    import_reference()
    ld = importlib.import_module("archnemesis.LineData_0")
    ls = importlib.import_module("archnemesis.lineshape")
    import archnemesis_dist_amd.forward_model as fmod
    true_fn = getattr(ld, "_ansfm_reference_pseudo_continuum", None) or ld.add_pseudo_continuum_monochromatic_absorption
    seen = []

    def spy(*a, **k):
        seen.append(1)
        return true_fn(*a, **k)

    monkeypatch.setattr(ld, "add_pseudo_continuum_monochromatic_absorption", spy)
    monkeypatch.setattr(ld, "_ansfm_reference_pseudo_continuum", None, raising=False)
    double = EngineDouble()
    monkeypatch.setattr(fmod, "get_engine", lambda device=0: double)
    monkeypatch.setattr(fmod, "DELEGATED", {})
    hook = fmod.install_gpu_pseudo_continuum(0)
    assert ld.add_pseudo_continuum_monochromatic_absorption is hook and ld._ansfm_reference_pseudo_continuum is spy
    yield dict(ld=ld, ls=ls, fmod=fmod, hook=hook, double=double, seen=seen, true_fn=true_fn)
    fmod.set_strict(False)


def _call(fn, shape_fn, d, out, **kw):
    return fn(d["wn_grid"], shape_fn, d["t_calc"], d["t_ref"], d["p_calc"], d["p_ref"], d["q_ratio"], d["isotopic_abundance"],
              d["isotopic_mass"], d["mol_mix_frac"], d["bparams"], d["centers"], d["widths"], d["sw_sum"], d["e_lower"], out, **kw)


@pytest.mark.parametrize("name,shape", [("regular", "voigt"), ("lorentz", "lorentz"), ("gaussian", "gaussian")])
def test_built_shapes_go_to_the_engine(hooked, golden_dir, name, shape):
    g = pc.load_golden(os.path.join(golden_dir, "lbl_pseudo_continuum.npz"))[name]
    N = g["centers"].shape[0]
    out, store, store_x = g["out0"].copy(), np.zeros((3, N)), np.zeros(N)
    hooked["fmod"].set_strict(True)                 # a delegation would raise
    _call(hooked["hook"], getattr(hooked["ls"], shape), g, out, store=store, store_x=store_x,
          store_y=np.zeros(7), store_z=np.zeros((2, out.size)), n_neighbour_bins=3)
    assert hooked["double"].calls == 1 and not hooked["seen"] and not hooked["fmod"].DELEGATED
    assert np.array_equal(out, g["out"]) and np.array_equal(store, g["store"]) and np.array_equal(store_x, g["store_x"])


def _delegation_cases(ls, g):
    """name -> (line shape, inputs, out, keywords) of calls the hook must hand to the reference"""
    N, nw = g["centers"].shape[0], g["wn_grid"].shape[0]
    swapped = dict(g); swapped["centers"] = g["centers"].copy(); swapped["centers"][[10, 11]] = swapped["centers"][[11, 10]]
    short = dict(g); short["wn_grid"] = g["wn_grid"][:N - 20].copy()
    return {
        "shape not built": (lambda dwn, ad, gl: ls.lorentz(dwn, ad, gl), g, np.zeros(nw), {}),
        "out not contiguous": (ls.voigt, g, np.zeros(2 * nw)[::2], {}),
        "out not float64": (ls.voigt, g, np.zeros(nw, dtype=np.float32), {}),
        "lower edges not ascending": (ls.voigt, swapped, np.zeros(nw), {}),
        "nine neighbour bins": (ls.voigt, g, np.zeros(nw), {"n_neighbour_bins": 9}),
        "no store_x, fewer grid points than bins": (ls.voigt, short, np.zeros(N - 20), {}),
    }


CASE_NAMES = ("shape not built", "out not contiguous", "out not float64", "lower edges not ascending", "nine neighbour bins",
              "no store_x, fewer grid points than bins")


@pytest.mark.parametrize("case", CASE_NAMES)
def test_cases_outside_the_gpu_path_go_to_the_reference(hooked, golden_dir, case):
    g = pc.load_golden(os.path.join(golden_dir, "lbl_pseudo_continuum.npz"))["regular"]
    shape_fn, d, out, kw = _delegation_cases(hooked["ls"], g)[case]
    fmod = hooked["fmod"]

    def run(fn, o):
        try:
            _call(fn, shape_fn, d, o, **kw)
            return None
        except IndexError as e:
            return e

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        err = run(hooked["hook"], out)
    assert hooked["double"].calls == 0 and len(hooked["seen"]) == 1
    assert sum(fmod.DELEGATED.values()) == 1
    # ... and what came back is what the reference's function does with the same call
    expect = out.copy(); expect[...] = 0
    err_ref = run(hooked["true_fn"], expect)
    assert (err is None) == (err_ref is None)
    if err is None:
        assert np.array_equal(out, expect) and np.any(out)
    fmod.set_strict(True)
    shape_fn, d, out, kw = _delegation_cases(hooked["ls"], g)[case]          # a fresh `out` of the same layout
    with pytest.raises(NotImplementedError):
        _call(hooked["hook"], shape_fn, d, out, **kw)
    assert hooked["double"].calls == 0 and len(hooked["seen"]) == 1
