"""install_gpu_surface against the REAL reference modules (build container only): Surface_0.calc_BRDF -- the class method, which
resolves calc_Hapke_BRDF / calc_OrenNayar_BRDF by global name at call time -- and ForwardModel_0.calc_brdf_matrix land on the
engine, here a test double answered by the NumPy restatement, so the argument mapping (the np.interp of the parameters, the
order of the ten Hapke arguments, MU as stored) and the memo are checked against the reference's own results in
tests/golden/brdf.npz.  The kernels behind the engine methods are covered on the GPU by tests/test_brdf_gpu.py."""
import importlib
import inspect
import os
import sys
import types

import numpy as np
import pytest

import brdf_cases as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_import import REFERENCE_ROOT, import_reference  # noqa: E402

pytestmark = [pytest.mark.needs_reference,
              pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE_ROOT, "archnemesis")), reason="reference tree not present")]


class EngineDouble:
    def __init__(self):
        self.points, self.matrices, self.fail = 0, 0, False

    def surface_brdf(self, lowbc, params, SOL_ANG, EMISS_ANG, AZI_ANG):
        self.points += 1
        if self.fail:
            raise ValueError("surface_brdf: ANSFM_ERR_INVALID: told to fail")
        return bc.surface_brdf_np(lowbc, params, SOL_ANG, EMISS_ANG, AZI_ANG)

    def brdf_matrix(self, lowbc, params, MU, NPHI, NF):
        self.matrices += 1
        if self.fail:
            raise ValueError("brdf_matrix: ANSFM_ERR_INVALID: told to fail")
        return bc.brdf_matrix_np(lowbc, params, MU, NPHI, NF)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return bc.load_golden(os.path.join(golden_dir, "brdf.npz"))


@pytest.fixture()
def hooked(monkeypatch):
    import_reference()
    su = importlib.import_module("archnemesis.Surface_0")
    fm = importlib.import_module("archnemesis.ForwardModel_0")
    import archnemesis_dist_amd.forward_model as fmod
    cls = fm.ForwardModel_0
    true = dict(hapke=getattr(su, "_ansfm_reference_calc_Hapke_BRDF", None) or su.calc_Hapke_BRDF,
                oren=getattr(su, "_ansfm_reference_calc_OrenNayar_BRDF", None) or su.calc_OrenNayar_BRDF,
                matrix=getattr(cls, "_ansfm_reference_calc_brdf_matrix", None) or cls.calc_brdf_matrix)
    seen = []

    def spy(kind):
        def f(*a, **k):
            seen.append(kind)
            return true[kind](*a, **k)
        return f

    monkeypatch.setattr(su, "calc_Hapke_BRDF", spy("hapke"))
    monkeypatch.setattr(su, "calc_OrenNayar_BRDF", spy("oren"))
    monkeypatch.setattr(cls, "calc_brdf_matrix", spy("matrix"))
    for obj, name in ((su, "_ansfm_reference_calc_Hapke_BRDF"), (su, "_ansfm_reference_calc_OrenNayar_BRDF"),
                      (cls, "_ansfm_reference_calc_brdf_matrix")):
        monkeypatch.setattr(obj, name, None, raising=False)
    double = EngineDouble()
    monkeypatch.setattr(fmod, "get_engine", lambda device=0: double)
    monkeypatch.setattr(fmod, "DELEGATED", {})
    monkeypatch.setattr(fmod, "ROUTES", {})
    hook = fmod.install_gpu_surface(0)
    assert cls.calc_brdf_matrix is hook and su.calc_Hapke_BRDF is not true["hapke"]
    yield dict(su=su, cls=cls, fmod=fmod, double=double, seen=seen)
    fmod.set_strict(False)


def _surface(su, g, coarse=False):
    """the case's surface on a spectral grid VEM; coarse: on every second wavenumber plus the last, so that np.interp works"""
    lowbc, P = int(g["lowbc"]), g["params"]
    wave = 1000.0 + 10.0 * np.arange(P.shape[1])
    keep = np.unique(np.r_[np.arange(0, wave.size, 2), wave.size - 1]) if coarse else np.arange(wave.size)
    s = su.Surface_0(GASGIANT=False, LOWBC=lowbc, GALB=-1.0, NEM=keep.size)
    s.VEM = wave[keep]
    if lowbc == 1:
        s.EMISSIVITY = 1.0 - P[0, keep]
    elif lowbc == 2:
        for name, row in zip(("SGLALB", "K", "BS0", "hs", "BC0", "hc", "ROUGHNESS", "G1", "G2", "F"), P):
            setattr(s, name, row[keep].copy())
    else:
        s.ALBEDO = P[0, keep].copy(); s.ROUGHNESS = P[1, keep].copy()
    return s, wave


def _scatter(g):
    return types.SimpleNamespace(NMU=len(g["MU"]), MU=g["MU"].copy(), NPHI=int(g["NPHI"]), NF=int(g["NF"]))


@pytest.mark.parametrize("name", ["hapke-opposition", "oren-nayar"])
def test_calc_brdf_gives_the_golden(hooked, golden, name):
    hooked["fmod"].set_strict(True)                    # a delegation would raise
    g = golden[name]
    s, wave = _surface(hooked["su"], g)
    got = s.calc_BRDF(wave, g["sol"], g["emi"], g["azi"])
    assert bc.deviation(got, g["ref"]) <= 1e-13
    assert hooked["double"].points == 1 and not hooked["seen"] and hooked["fmod"].ROUTES == {"brdf points": 1}


def test_calc_brdf_matrix_gives_the_golden_and_remembers(hooked, golden):
    fmod, double, cls = hooked["fmod"], hooked["double"], hooked["cls"]
    fmod.set_strict(True)
    g = golden["m-5-101-2"]
    s, wave = _surface(hooked["su"], g)
    first = cls.calc_brdf_matrix(None, WAVEC=wave, Scatter=_scatter(g), Surface=s)
    assert bc.deviation(first, g["ref"]) <= 1e-13
    assert double.matrices == 1 and fmod.ROUTES == {"brdf matrix": 1}
    keep = first.copy()
    first[...] = -1.0                                  # what the caller does with a result does not reach the memo
    again = cls.calc_brdf_matrix(None, WAVEC=wave, Scatter=_scatter(g), Surface=s)
    assert double.matrices == 1 and fmod.ROUTES == {"brdf matrix": 1, "brdf matrix (memo)": 1}
    assert again is not first and np.array_equal(again, keep)
    again[...] = 7.0
    third = cls.calc_brdf_matrix(None, WAVEC=wave, Scatter=_scatter(g), Surface=s)
    assert double.matrices == 1 and np.array_equal(third, keep)
    # one changed bit, in any argument, reaches the engine
    s.hc = s.hc.copy(); s.hc[1] = np.nextafter(s.hc[1], 2.0)
    cls.calc_brdf_matrix(None, WAVEC=wave, Scatter=_scatter(g), Surface=s)
    sc = _scatter(g); sc.NF = 3
    cls.calc_brdf_matrix(None, WAVEC=wave, Scatter=sc, Surface=s)
    sc = _scatter(g); sc.MU[0] = np.nextafter(sc.MU[0], 1.0)
    cls.calc_brdf_matrix(None, WAVEC=wave, Scatter=sc, Surface=s)
    assert double.matrices == 4 and fmod.ROUTES["brdf matrix"] == 4 and not hooked["seen"] and not fmod.DELEGATED


def test_parameters_are_interpolated_on_the_host(hooked, golden):
    """a surface given on a coarser grid than the calculation's: the engine is handed np.interp's values, as calc_BRDF
    (:952-961) hands them to calc_Hapke_BRDF"""
    g = golden["m-5-101-2"]
    s, wave = _surface(hooked["su"], g, coarse=True)
    got = hooked["cls"].calc_brdf_matrix(None, WAVEC=wave, Scatter=_scatter(g), Surface=s)
    P = np.stack([np.interp(wave, s.VEM, getattr(s, n)) for n in ("SGLALB", "K", "BS0", "hs", "BC0", "hc", "ROUGHNESS", "G1", "G2", "F")])
    assert not np.array_equal(P, g["params"])
    assert np.array_equal(got, bc.brdf_matrix_np(2, P, g["MU"], 101, 2))


@pytest.mark.parametrize("name", ["m-lambert", "m-oren-nayar"])
def test_other_boundaries_reach_the_reference(hooked, golden, name):
    fmod = hooked["fmod"]
    fmod.set_strict(True)                              # ... and that is no delegation
    g = golden[name]
    s, wave = _surface(hooked["su"], g)
    got = hooked["cls"].calc_brdf_matrix(None, WAVEC=wave, Scatter=_scatter(g), Surface=s)
    assert np.array_equal(got, g["ref"])
    assert hooked["seen"] == ["matrix"] and hooked["double"].matrices == 0 and not fmod.DELEGATED and not fmod.ROUTES


def test_engine_error_goes_to_the_reference(hooked, golden):
    fmod, double = hooked["fmod"], hooked["double"]
    double.fail = True
    g = dict(golden["m-5-101-2"])
    g["params"] = g["params"][:, :1]                   # one wavenumber: the un-jitted reference is slow
    s, wave = _surface(hooked["su"], g)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = hooked["cls"].calc_brdf_matrix(None, WAVEC=wave, Scatter=_scatter(g), Surface=s)
    assert np.array_equal(got, golden["m-5-101-2"]["ref"][:1])
    assert hooked["seen"] == ["matrix", "hapke"] and sum(fmod.DELEGATED.values()) == 2 and not fmod.ROUTES
    fmod.set_strict(True)
    with pytest.raises(NotImplementedError):
        hooked["cls"].calc_brdf_matrix(None, WAVEC=wave, Scatter=_scatter(g), Surface=s)


def test_install_all_names_the_hook():
    import archnemesis_dist_amd.forward_model as fmod
    assert "install_gpu_surface" in inspect.getsource(fmod.install_all)
