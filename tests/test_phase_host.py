"""Aerosol phase functions on the calculation grid, without a GPU: the NumPy restatement of tests/phase_cases.py against the
reference's results in tests/golden/phase.npz (tools/golden/gen_golden_phase.py), the C-ABI's declarations, and
forward_model.install_gpu_phase against the REAL reference class (build container only) with an engine double answered by
the restatement: the argument mapping, the reference's two ValueErrors, the delegations and strict mode.  The kernels behind
the engine methods are covered on the GPU by tests/test_phase_gpu.py and tests/test_phase_fused_gpu.py."""
import importlib
import inspect
import os
import sys
import warnings

import numpy as np
import pytest

import phase_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_import import REFERENCE_ROOT, import_reference  # noqa: E402

GOLDEN = pc.load_golden(os.path.join(ROOT, "tests", "golden", "phase.npz"))
CASES = ("hg-2x1", "hg-7pop", "mie-nodes", "mie-paths", "lp-1", "lp-2", "lp-36", "ray", "um")
NEW = ("ansfm_calc_phase", "ansfm_calc_phase_ray", "ansfm_phase_last", "ansfm_upload_phase", "ansfm_phase_from_source",
       "ansfm_cirsrad_ck_singlescatt_batch_src", "ansfm_cirsrad_ck_scatter_batch_src")



def needs_reference(fn):
    fn = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE_ROOT, "archnemesis")), reason="reference tree not present")(fn)
    return pytest.mark.needs_reference(fn)


def test_golden_holds_every_case():
    assert set(GOLDEN) == set(CASES)
    fresh = pc.golden_cases()
    for name in CASES:                      # the inputs are those phase_cases builds today
        for k, v in fresh[name].items():
            assert np.array_equal(GOLDEN[name][k], v), (name, k)


@pytest.mark.parametrize("name", CASES)
def test_restatement_against_the_reference(name):
    d = GOLDEN[name]
    got, ref, ulp = pc.evaluate_np(d), d["ref"], float(d["ulp"])
    assert got.shape == ref.shape
    dev = pc.deviation(got, ref)
    print("%s: deviation %.2e, 4 x ulp %.2e" % (name, dev, 4 * ulp))
    if int(d.get("imie", -1)) in pc.EXACT_KINDS:
        assert np.array_equal(got, ref)
    else:
        assert dev <= 4 * ulp
    if "hg" in d:                           # the slots of the scattering array
        assert np.array_equal(pc.hg_on_grid(d["swave"], d["tab"], d["wave"]), d["hg"])


@pytest.mark.parametrize("name", CASES)
def test_sixteen_ulp_stay_below_the_parity_bar(name):
    assert float(GOLDEN[name]["ulp"]) <= 1e-6 / 16


def test_scattering_array_of_the_restatement():
    d = GOLDEN["mie-nodes"]
    arr = pc.phasarr_np(1, d["swave"], d["ttab"], d["tab"], d["ttab"], d["wave"])
    assert arr.shape == (2, d["wave"].shape[0], 2, 5)
    ref = pc.calc_phase_np(1, d["swave"], d["ttab"], d["tab"], d["ttab"], d["wave"])
    assert np.array_equal(arr[:, :, 0, ::-1], np.transpose(ref, (2, 0, 1)))
    assert np.array_equal(arr[0, 0, 1, ::-1], np.cos(d["ttab"] * np.pi / 180))
    h = GOLDEN["um"]
    arr = pc.phasarr_np(0, h["swave"], h["ttab"], h["tab"], h["theta"], h["wave"])
    assert np.array_equal(arr[:, :, 0, :3], np.transpose(h["hg"], (1, 2, 0))) and not arr[:, :, 0, 3:].any()


def test_header_declares_the_entries():
    from archnemesis_dist_amd import _lib
    header = open(os.path.join(ROOT, "include", "ansfm.h")).read()
    protos = _lib.prototypes(header)
    import ctypes as C
    for name in NEW + ("ansfm_phasarr_from_source",):
        assert name in protos, name
        assert protos[name][0] is C.c_int
    assert protos["ansfm_calc_phase"][1] == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert protos["ansfm_upload_phase"][1] == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    # the fused entries: the arguments of the _cont entries with the phase function replaced
    ss, ss0 = protos["ansfm_cirsrad_ck_singlescatt_batch_src"][1], protos["ansfm_cirsrad_ck_singlescatt_batch_cont"][1]
    assert ss == ss0
    ms, ms0 = protos["ansfm_cirsrad_ck_scatter_batch_src"][1], protos["ansfm_cirsrad_ck_scatter_batch_cont"][1]
    assert len(ms) == len(ms0) + 1 and ms[:18] == ms0[:18] and ms[18:20] == [C.c_void_p, C.c_void_p] and ms[20:] == ms0[19:]


def test_library_exports_the_entries_and_keeps_its_abi():
    from archnemesis_dist_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.ansfm_abi_version() == 1


def test_engine_has_the_methods():
    from archnemesis_dist_amd.engine import AnsfmEngine
    for name in ("calc_phase", "calc_phase_ray", "upload_phase", "phase_from_source", "phase_last",
                 "cirsrad_ck_singlescatt_batch_src", "cirsrad_ck_scatter_batch_src"):
        assert callable(getattr(AnsfmEngine, name)), name


def test_install_all_does_not_name_the_hook():
    import archnemesis_dist_amd.forward_model as fmod
    assert callable(fmod.install_gpu_phase)
    assert "install_gpu_phase" not in inspect.getsource(fmod.install_all)


# ---- install_gpu_phase against the reference class ---------------------------------------------------------------------
class EngineDouble:
    def __init__(self):
        self.calls, self.ray_calls, self.fail, self.last = 0, 0, None, None

    def calc_phase(self, imie, SWAVE, THETA_TAB, tab, theta, WAVEC):
        self.calls += 1
        self.last = (imie, SWAVE, THETA_TAB, tab, theta, WAVEC)
        if self.fail:
            raise self.fail
        return pc.calc_phase_np(imie, SWAVE, THETA_TAB, tab, theta, WAVEC)

    def calc_phase_ray(self, theta):
        self.ray_calls += 1
        return pc.calc_phase_ray_np(theta)


@pytest.fixture()
def hooked(monkeypatch):
    import_reference()
    sc = importlib.import_module("archnemesis.Scatter_0")
    import archnemesis_dist_amd.forward_model as fmod
    cls = sc.Scatter_0
    true_phase = getattr(cls, "_ansfm_reference_calc_phase", None) or cls.calc_phase
    true_ray = getattr(cls, "_ansfm_reference_calc_phase_ray", None) or cls.calc_phase_ray
    seen = []

    def spy(self, Theta, Wave):
        seen.append(np.shape(Theta))
        return true_phase(self, Theta, Wave)

    monkeypatch.setattr(cls, "calc_phase", spy)
    monkeypatch.setattr(cls, "calc_phase_ray", true_ray)
    monkeypatch.setattr(cls, "_ansfm_reference_calc_phase", None, raising=False)
    monkeypatch.setattr(cls, "_ansfm_reference_calc_phase_ray", None, raising=False)
    double = EngineDouble()
    monkeypatch.setattr(fmod, "get_engine", lambda device=0: double)
    monkeypatch.setattr(fmod, "DELEGATED", {})
    monkeypatch.setattr(fmod, "ROUTES", {})
    hooks = fmod.install_gpu_phase(0)
    assert cls.calc_phase is hooks[0] and cls.calc_phase_ray is hooks[1] and cls._ansfm_reference_calc_phase is spy
    yield dict(sc=sc, fmod=fmod, double=double, seen=seen, true_phase=true_phase, true_ray=true_ray)
    fmod.set_strict(False)


def _scatter(sc, d):
    imie, tab = int(d["imie"]), d["tab"]
    s = sc.Scatter_0(IMIE=imie, NDUST=tab.shape[2])
    s.NWAVE = d["swave"].shape[0]
    s.WAVE = d["swave"].copy()
    if imie == 0:
        s.F, s.G1, s.G2 = tab[0].copy(), tab[1].copy(), tab[2].copy()
    elif imie == 1:
        s.NTHETA, s.THETA, s.PHASE = d["ttab"].shape[0], d["ttab"].copy(), tab.copy()
    else:
        s.NLPOL, s.WLPOL = tab.shape[1], tab.copy()
    return s


@needs_reference
@pytest.mark.parametrize("name", ["hg-7pop", "mie-paths", "lp-36", "um"])
def test_hook_maps_the_arguments(hooked, name):
    sc, fmod, d = hooked["sc"], hooked["fmod"], GOLDEN[name]
    fmod.set_strict(True)                           # a delegation would raise
    got = _scatter(sc, d).calc_phase(d["theta"].copy(), d["wave"].copy())
    assert hooked["double"].calls == 1 and not hooked["seen"] and fmod.ROUTES == {"phase": 1}
    imie, SW, TT, tab, th, wv = hooked["double"].last
    assert imie == int(d["imie"]) and np.array_equal(SW, d["swave"]) and np.array_equal(tab, d["tab"])
    assert np.array_equal(th, d["theta"]) and np.array_equal(wv, d["wave"]) and (imie != 1 or np.array_equal(TT, d["ttab"]))
    if imie == 1:
        assert np.array_equal(got, d["ref"])
    else:
        assert pc.deviation(got, d["ref"]) <= 4 * float(d["ulp"])
    ray = _scatter(sc, d).calc_phase_ray(GOLDEN["ray"]["theta"].copy())
    assert hooked["double"].ray_calls == 1 and fmod.ROUTES == {"phase": 2}
    assert pc.deviation(ray, GOLDEN["ray"]["ref"]) <= 4 * float(GOLDEN["ray"]["ulp"])


@needs_reference
def test_hook_keeps_the_reference_errors(hooked):
    sc, fmod = hooked["sc"], hooked["fmod"]
    fmod.set_strict(True)                           # neither is a delegation
    d = GOLDEN["mie-nodes"]
    s = _scatter(sc, d)
    for wave in (d["wave"] * 0.99, d["wave"] * 1.01):
        with pytest.raises(ValueError) as mine:
            s.calc_phase(d["theta"].copy(), wave)
        with pytest.raises(ValueError) as ref:
            hooked["true_phase"](s, d["theta"].copy(), wave)
        assert str(mine.value) == str(ref.value) and "does not fully cover" in str(mine.value)
    short = _scatter(sc, dict(d, ttab=d["ttab"][1:-1], tab=d["tab"][:, 1:-1]))
    for theta in (np.array([10.0, 60.0]), np.array([60.0, 150.0])):
        with pytest.raises(ValueError) as mine:
            short.calc_phase(theta, d["wave"].copy())
        with pytest.raises(ValueError) as ref:
            hooked["true_phase"](short, theta, d["wave"].copy())
        assert str(mine.value) == str(ref.value) and "interpolation range" in str(mine.value)
    assert hooked["double"].calls == 0 and not fmod.DELEGATED and not fmod.ROUTES


@needs_reference
def test_hook_delegates(hooked):
    sc, fmod, d = hooked["sc"], hooked["fmod"], GOLDEN["um"]
    ref = d["ref"]

    def delegated(s, theta, wave, count):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            out = s.calc_phase(theta, wave)
        assert sum(fmod.DELEGATED.values()) == count and len(hooked["seen"]) == count
        return out

    # a descending Scatter.WAVE: interp1d sorts it, the kernel would not
    s = _scatter(sc, d)
    s.WAVE = s.WAVE[::-1].copy(); s.F, s.G1, s.G2 = s.F[::-1].copy(), s.G1[::-1].copy(), s.G2[::-1].copy()
    assert np.array_equal(delegated(s, d["theta"].copy(), d["wave"].copy(), 1), ref)
    # arrays that are not float64
    assert delegated(_scatter(sc, d), d["theta"].copy(), d["wave"].astype(np.float32), 2).shape == ref.shape
    s = _scatter(sc, d); s.F = s.F.astype(np.float32)
    delegated(s, d["theta"].copy(), d["wave"].copy(), 3)
    # what the engine refuses as unsupported (more than 7 populations through a resident source)
    hooked["double"].fail = NotImplementedError("upload_phase: ANSFM_ERR_UNSUPPORTED: more than 7 aerosol populations")
    assert np.array_equal(delegated(_scatter(sc, d), d["theta"].copy(), d["wave"].copy(), 4), ref)
    assert hooked["double"].calls == 1 and not fmod.ROUTES
    hooked["double"].fail = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sc.Scatter_0().calc_phase_ray(np.array([10, 20]))
    assert sum(fmod.DELEGATED.values()) == 5
    # strict mode turns every one of them into an error
    fmod.set_strict(True)
    s = _scatter(sc, d); s.F = s.F.astype(np.float32)
    with pytest.raises(NotImplementedError):
        s.calc_phase(d["theta"].copy(), d["wave"].copy())
    with pytest.raises(NotImplementedError):
        sc.Scatter_0().calc_phase_ray(np.array([10, 20]))
