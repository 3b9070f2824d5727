"""install_gpu_mie against the REAL reference module (build container only): Scatter_0.makephase(idust, iscat, pars) -- the
class method, which resolves the module-level makephase at call time -- lands on the engine for iscat 1 .. 4, here a test
double answered by the NumPy restatement, so the argument mapping and the memo are checked against the reference's own
result.  The kernels behind the engine method are covered on the GPU by tests/test_mie_gpu.py."""
import importlib
import os
import sys
import warnings

import numpy as np
import pytest

import mie_cases as mc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_import import REFERENCE_ROOT, import_reference  # noqa: E402

pytestmark = [pytest.mark.needs_reference,
              pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE_ROOT, "archnemesis")), reason="reference tree not present")]

RS = (0.05, 0.55, 0.05)                   # a closed range of a few radii: the un-jitted reference is slow


class EngineDouble:
    def __init__(self):
        self.calls = 0
        self.fail = False

    def mie_makephase(self, wavel, iscat, dsize, rs, refindx, theta, radius_block=None, return_counts=False):
        self.calls += 1
        if self.fail:
            raise ValueError("mie_makephase: ANSFM_ERR_INVALID: told to fail")
        return mc.makephase_np(wavel, iscat, dsize, rs, refindx, theta, return_counts=return_counts)


@pytest.fixture()
def hooked(monkeypatch):
    import_reference()
    sc = importlib.import_module("archnemesis.Scatter_0")
    import archnemesis_dist_amd.forward_model as fmod
    true_fn = getattr(sc, "_ansfm_reference_makephase", None) or sc.makephase
    seen = []

    def spy(*a, **k):
        seen.append(int(a[1]))
        return true_fn(*a, **k)

    monkeypatch.setattr(sc, "makephase", spy)
    monkeypatch.setattr(sc, "_ansfm_reference_makephase", None, raising=False)
    double = EngineDouble()
    monkeypatch.setattr(fmod, "get_engine", lambda device=0: double)
    monkeypatch.setattr(fmod, "DELEGATED", {})
    monkeypatch.setattr(fmod, "ROUTES", {})
    hook = fmod.install_gpu_mie(0)
    assert sc.makephase is hook and sc._ansfm_reference_makephase is spy
    yield dict(sc=sc, fmod=fmod, hook=hook, double=double, seen=seen, true_fn=true_fn)
    fmod.set_strict(False)


def _scatter(sc):
    """two aerosol populations on a descending wavenumber grid (so that the class method's sort permutes), explicit phase
    functions (IMIE = 1) at angles on both sides of 90 degrees"""
    theta = np.array([0.0, 30.0, 90.0, 150.0, 180.0])
    s = sc.Scatter_0(ISPACE=0, IMIE=1, NDUST=2, NTHETA=theta.shape[0], THETA=theta)
    s.initialise_arrays(2, 3, theta.shape[0])
    s.WAVE = np.array([12500.0, 10000.0, 5000.0])          # 0.8, 1, 2 um
    s.WAVER = np.array([0.5, 1.0, 3.0]); s.REFIND_REAL = np.array([1.40, 1.45, 1.50]); s.REFIND_IM = np.array([0.01, 0.02, 0.05])
    return s


def _state(s):
    return {k: getattr(s, k).copy() for k in ("KEXT", "KSCA", "SGLALB", "PHASE")}


def test_class_method_gives_the_reference_result(hooked, monkeypatch):
    sc, fmod = hooked["sc"], hooked["fmod"]
    fmod.set_strict(True)                           # a delegation would raise
    a = _scatter(sc)
    a.makephase(1, 2, [0.3, 0.4], rs=RS)
    assert hooked["double"].calls == 1 and not hooked["seen"] and fmod.ROUTES == {"mie": 1}
    monkeypatch.setattr(sc, "makephase", hooked["true_fn"])
    b = _scatter(sc)
    b.makephase(1, 2, [0.3, 0.4], rs=RS)
    for k, v in _state(b).items():
        assert np.any(v[..., 1]) and not np.any(v[..., 0]), k
        np.testing.assert_allclose(getattr(a, k), v, rtol=1e-12, atol=0, err_msg=k)


def test_memo_returns_copies_and_sees_every_argument(hooked):
    sc, fmod, double = hooked["sc"], hooked["fmod"], hooked["double"]
    a = _scatter(sc)
    a.makephase(0, 2, [0.3, 0.4], rs=RS)
    first = _state(a)
    a.PHASE[...] = -1.0                             # what the caller does with the first result ...
    wavel = np.sort(1.0e4 / a.WAVE)
    refindx = np.stack([np.interp(wavel, a.WAVER, a.REFIND_REAL), np.interp(wavel, a.WAVER, a.REFIND_IM)], axis=1)
    args = (wavel, 2, np.array([0.3, 0.4, 0.0]), np.array(RS), refindx, np.array([0.0, 30.0, 90.0]))
    r1 = hooked["hook"](*args)
    assert double.calls == 1 and fmod.ROUTES == {"mie": 1, "mie (memo)": 1}
    r1[3][...] = 7.0; r1[0][...] = 7.0              # ... or with a remembered one does not reach the memo
    b = _scatter(sc)
    b.makephase(0, 2, [0.3, 0.4], rs=RS)
    assert double.calls == 1 and fmod.ROUTES["mie (memo)"] == 2
    for k, v in _state(b).items():
        assert np.array_equal(v, first[k]), k
    # one changed parameter, in any argument, reaches the engine
    b.makephase(0, 2, [0.3, np.nextafter(0.4, 1.0)], rs=RS)
    assert double.calls == 2
    b.REFIND_IM = b.REFIND_IM * (1 + 1e-15)
    b.makephase(0, 2, [0.3, 0.4], rs=RS)
    assert double.calls == 3 and fmod.ROUTES["mie"] == 3 and not hooked["seen"] and not fmod.DELEGATED


def test_closed_forms_are_forwarded_without_a_delegation(hooked):
    sc, fmod = hooked["sc"], hooked["fmod"]
    fmod.set_strict(True)
    a = _scatter(sc)
    a.makephase(0, 6, [0.6, 0.7, -0.3])
    assert hooked["seen"] == [6] and hooked["double"].calls == 0 and not fmod.DELEGATED and not fmod.ROUTES
    assert np.all(a.PHASE[:, :, 0] > 0)


def test_engine_error_goes_to_the_reference(hooked):
    sc, fmod, double = hooked["sc"], hooked["fmod"], hooked["double"]
    double.fail = True
    a = _scatter(sc)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a.makephase(0, 2, [0.3, 0.4], rs=RS)
    assert double.calls == 1 and hooked["seen"] == [2] and sum(fmod.DELEGATED.values()) == 1 and not fmod.ROUTES
    assert np.all(a.KEXT[:, 0] > 0)
    fmod.set_strict(True)
    with pytest.raises(NotImplementedError):
        a.makephase(0, 2, [0.3, 0.4], rs=RS)
    assert double.calls == 2 and hooked["seen"] == [2]


def test_install_all_names_the_hook():
    import archnemesis_dist_amd.forward_model as fmod
    import inspect
    assert "install_gpu_mie" in inspect.getsource(fmod.install_all)


def test_states_of_a_jacobian_with_a_model_444_variable(hooked):
    """What the staged Jacobian route does with a model-444 variable, at the level of the model: every one of the NX + 1 states
    runs Model444.calculate (model_444.py:78 -> Scatter.makephase :154) from its slice of the state vector.  The states that
    perturb another variable repeat the unperturbed aerosol bit for bit: the engine is reached once per distinct aerosol state,
    the memo answers the rest, and every state's KEXT / PHASE are those of its own slice."""
    sc, fmod, double = hooked["sc"], hooked["fmod"], hooked["double"]
    Model444 = importlib.import_module("archnemesis.Models.PreRTModels.model_444").Model444
    fmod.set_strict(True)
    haze = {"WAVE": np.array([0.5, 1.0, 3.0]), "NREAL": 1.4, "WAVE_REF": 1.0, "WAVE_NORM": 1.0}
    x0 = np.log(np.array([0.3, 0.4, 0.01]))
    states = [x0.copy() for _ in range(9)]                    # state 0 and 8 perturbed ones, 3 of them in the 444 slice
    for k, j in ((2, 0), (5, 1), (7, 2)):
        states[k][j] *= 1.05
    got = []
    for x in states:
        s = _scatter(sc)
        s.initialise_arrays(2, 2, s.NTHETA)
        s.WAVE = np.array([10000.0, 5000.0])                  # 1 and 2 um
        Model444.calculate(s, 1, 2, x, haze)
        got.append((s.KEXT.copy(), s.PHASE.copy()))
    assert fmod.ROUTES == {"mie": 4, "mie (memo)": 5} and double.calls == 4 and not fmod.DELEGATED and not hooked["seen"]
    for k, (kext, phase) in enumerate(got):
        same = k not in (2, 5, 7)
        assert np.array_equal(kext, got[0][0]) == same, k
        assert np.array_equal(phase, got[0][1]) == same, k
        assert np.all(phase[:, :, 1] > 0)
