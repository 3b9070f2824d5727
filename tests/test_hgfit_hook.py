"""install_gpu_hg_fit against the REAL reference module (build container only): with IMIE = 0 the class method
Scatter_0.makephase(idust, iscat, pars) -- which resolves the module-level makephase and subfithgm at call time -- lands on the
engine twice, here a test double answered by the NumPy restatements (the fit in the kernel's order), so the argument mapping
and the memo are checked against the reference's own result.  The kernel behind the engine method is covered on the GPU by
tests/test_hgfit_gpu.py.  Then the memo capacity of a staged Jacobian: a stand-in for the forward model walks
`for geometry: for state` over 12 distinct aerosol states."""
import importlib
import inspect
import os
import sys
import warnings

import numpy as np
import pytest

import hgfit_cases as hc
import mie_cases as mc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_import import REFERENCE_ROOT, import_reference  # noqa: E402

pytestmark = [pytest.mark.needs_reference,
              pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE_ROOT, "archnemesis")), reason="reference tree not present")]

RS = (0.05, 0.55, 0.05)                   # a closed range of a few radii: the un-jitted reference is slow
# the double answers with the restatement in the kernel's order, which tools/golden/gen_golden_hgfit.py holds to 1e-8 of the
# reference on every case (a case above it is replaced): the bound of a fit that is no case
BOUND = 1e-8


class EngineDouble:
    def __init__(self):
        self.calls = 0
        self.mie_calls = 0
        self.fail = False

    def mie_makephase(self, wavel, iscat, dsize, rs, refindx, theta, radius_block=None, return_counts=False):
        self.mie_calls += 1
        return mc.makephase_np(wavel, iscat, dsize, rs, refindx, theta, return_counts=return_counts)

    def hg_fit(self, theta, phase, return_counts=False):
        self.calls += 1
        if self.fail:
            raise ValueError("hg_fit: ANSFM_ERR_INVALID: told to fail")
        return hc.subfithgm_np(theta, phase, order="kernel", return_counts=return_counts)


@pytest.fixture()
def hooked(monkeypatch):
    import_reference()
    sc = importlib.import_module("archnemesis.Scatter_0")
    import archnemesis_dist_amd.forward_model as fmod
    true_fn = getattr(sc, "_ansfm_reference_subfithgm", None) or sc.subfithgm
    true_mie = getattr(sc, "_ansfm_reference_makephase", None) or sc.makephase
    seen = []

    def spy(theta, phase):
        seen.append(phase.shape)
        return true_fn(theta, phase)

    monkeypatch.setattr(sc, "subfithgm", spy)
    monkeypatch.setattr(sc, "_ansfm_reference_subfithgm", None, raising=False)
    monkeypatch.setattr(sc, "makephase", true_mie)
    monkeypatch.setattr(sc, "_ansfm_reference_makephase", None, raising=False)
    double = EngineDouble()
    monkeypatch.setattr(fmod, "get_engine", lambda device=0: double)
    monkeypatch.setattr(fmod, "DELEGATED", {})
    monkeypatch.setattr(fmod, "ROUTES", {})
    monkeypatch.setattr(fmod, "MIE_MEMO_ENTRIES", 8)
    monkeypatch.setattr(fmod, "HG_FIT_MEMO_ENTRIES", 8)
    fmod.install_gpu_mie(0)
    hook = fmod.install_gpu_hg_fit(0)
    assert sc.subfithgm is hook and sc._ansfm_reference_subfithgm is spy
    yield dict(sc=sc, fmod=fmod, hook=hook, double=double, seen=seen, true_fn=true_fn, true_mie=true_mie)
    fmod.set_strict(False)


def _scatter(sc):
    """two aerosol populations on a descending wavenumber grid (so that the class method's sort permutes), Henyey-Greenstein
    parameters (IMIE = 0), angles on both sides of 90 degrees"""
    theta = np.array([0.0, 30.0, 90.0, 150.0, 180.0])
    s = sc.Scatter_0(ISPACE=0, IMIE=0, NDUST=2, NTHETA=theta.shape[0], THETA=theta)
    s.initialise_arrays(2, 3, theta.shape[0])
    s.WAVE = np.array([12500.0, 10000.0, 5000.0])          # 0.8, 1, 2 um
    s.WAVER = np.array([0.5, 1.0, 3.0]); s.REFIND_REAL = np.array([1.40, 1.45, 1.50]); s.REFIND_IM = np.array([0.01, 0.02, 0.05])
    return s


def _state(s):
    return {k: getattr(s, k).copy() for k in ("KEXT", "KSCA", "F", "G1", "G2")}


def test_class_method_gives_the_reference_result(hooked, monkeypatch):
    sc, fmod = hooked["sc"], hooked["fmod"]
    fmod.set_strict(True)                           # a delegation would raise
    a = _scatter(sc)
    a.makephase(1, 2, [0.3, 0.4], rs=RS)
    assert hooked["double"].calls == 1 and not hooked["seen"] and fmod.ROUTES == {"mie": 1, "hg fit": 1}
    monkeypatch.setattr(sc, "makephase", hooked["true_mie"])
    monkeypatch.setattr(sc, "subfithgm", hooked["true_fn"])
    b = _scatter(sc)
    b.makephase(1, 2, [0.3, 0.4], rs=RS)
    for k in ("F", "G1", "G2"):
        v = getattr(b, k)
        assert np.any(v[:, 1]) and not np.any(v[:, 0]), k
        assert len(set(v[:, 1])) == 3                # three wavelengths, three fits: a permutation would show
        dev = np.max(np.abs(getattr(a, k)[:, 1] - v[:, 1]) / np.abs(v[:, 1]))
        print("%s: %.2e" % (k, dev))
        assert dev <= BOUND, (k, dev)
    np.testing.assert_allclose(a.KEXT, b.KEXT, rtol=1e-12, atol=0)


def test_memo_returns_copies_and_sees_every_argument(hooked):
    sc, fmod, double, hook = hooked["sc"], hooked["fmod"], hooked["double"], hooked["hook"]
    g = hc.load_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hgfit.npz"))["lognormal-41"]
    theta, phase = g["theta"], g["phase"][:2]
    first = hook(theta, phase)
    assert double.calls == 1 and fmod.ROUTES == {"hg fit": 1}
    kept = [a.copy() for a in first]
    first[0][...] = 7.0; first[3][...] = 7.0         # what a caller does with a result does not reach the memo
    second = hook(theta.copy(), phase.copy())
    assert double.calls == 1 and fmod.ROUTES == {"hg fit": 1, "hg fit (memo)": 1}
    for a, b in zip(second, kept):
        assert np.array_equal(a, b)
    second[1][...] = -1.0                            # ... nor with a remembered one
    third = hook(theta, phase)
    assert double.calls == 1 and np.array_equal(third[1], kept[1])
    # one changed element, in either argument, reaches the engine
    p2 = phase.copy(); p2[1, 40] = np.nextafter(p2[1, 40], np.inf)
    hook(theta, p2)
    assert double.calls == 2
    t2 = theta.copy(); t2[3] = np.nextafter(t2[3], np.inf)
    hook(t2, phase)
    assert double.calls == 3 and fmod.ROUTES == {"hg fit": 3, "hg fit (memo)": 2} and not hooked["seen"] and not fmod.DELEGATED


def test_engine_error_goes_to_the_reference(hooked):
    sc, fmod, double = hooked["sc"], hooked["fmod"], hooked["double"]
    double.fail = True
    a = _scatter(sc)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a.makephase(0, 2, [0.3, 0.4], rs=RS)
    assert double.calls == 1 and hooked["seen"] == [(3, 5)] and sum(fmod.DELEGATED.values()) == 1 and fmod.ROUTES == {"mie": 1}
    assert np.all(a.F[:, 0] > 0) and np.all(a.G2[:, 0] < 0)
    fmod.set_strict(True)
    with pytest.raises(NotImplementedError):
        a.makephase(0, 2, [0.3, 0.4], rs=RS)
    assert double.calls == 2 and hooked["seen"] == [(3, 5)]


def test_refused_arguments_are_delegated(hooked):
    fmod, double, hook = hooked["fmod"], hooked["double"], hooked["hook"]
    theta = np.array([0.0, 90.0, 180.0])
    phase = np.array([[3.0, 0.8, 0.5]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ref = hook(theta, phase.astype(np.float32))                 # not float64
        with pytest.raises(IndexError):
            hook(theta, phase[0])                                   # not 2-D: the reference fails its own way
    assert double.calls == 0 and hooked["seen"] == [(1, 3), (3,)] and sum(fmod.DELEGATED.values()) == 2
    assert 0.0 < ref[0][0] < 1.0
    fmod.set_strict(True)
    n = fmod.HG_FIT_NPHASE_CAP + 1
    with pytest.raises(NotImplementedError, match="angles"):
        hook(np.linspace(0.0, 180.0, n), np.ones((1, n)))
    with pytest.raises(NotImplementedError):
        hook(theta, phase.astype(np.float32))
    assert double.calls == 0


def test_install_all_names_the_hook():
    import archnemesis_dist_amd.forward_model as fmod
    src = inspect.getsource(fmod.install_all)
    assert "install_gpu_hg_fit" in src and "install_gpu_mie" in src


def test_states_of_a_jacobian_with_a_model_444_variable(hooked):
    """The sequence of tests/test_mie_hook.py with IMIE = 0: nine states, three of them with a perturbed aerosol.  Mie
    integration and fit reach the engine once per distinct aerosol state, the memos answer the rest."""
    sc, fmod, double = hooked["sc"], hooked["fmod"], hooked["double"]
    Model444 = importlib.import_module("archnemesis.Models.PreRTModels.model_444").Model444
    fmod.set_strict(True)
    haze = {"WAVE": np.array([0.5, 1.0, 3.0]), "NREAL": 1.4, "WAVE_REF": 1.0, "WAVE_NORM": 1.0}
    x0 = np.log(np.array([0.3, 0.4, 0.01]))
    states = [x0.copy() for _ in range(9)]
    for k, j in ((2, 0), (5, 1), (7, 2)):
        states[k][j] *= 1.05
    got = []
    for x in states:
        s = _scatter(sc)
        s.initialise_arrays(2, 2, s.NTHETA)
        s.WAVE = np.array([10000.0, 5000.0])                  # 1 and 2 um
        Model444.calculate(s, 1, 2, x, haze)
        got.append((s.F.copy(), s.G1.copy(), s.G2.copy()))
    assert fmod.ROUTES == {"mie": 4, "mie (memo)": 5, "hg fit": 4, "hg fit (memo)": 5}
    assert double.calls == 4 and double.mie_calls == 4 and not fmod.DELEGATED and not hooked["seen"]
    for k, fg in enumerate(got):
        same = k not in (2, 5, 7)
        assert all(np.array_equal(a, b) for a, b in zip(fg, got[0])) == same, k
        assert np.all(fg[0][:, 1] > 0) and np.all(fg[2][:, 1] < 0) and not np.any(fg[0][:, 0])


# ---- memo capacity of a staged Jacobian ---------------------------------------------------------------------------------
class AerosolModel:
    """what makes a model count: its class calls Scatter.makephase (Models/PreRTModels/model_444.py:154)"""
    n_state_vector_entries = 11

    @classmethod
    def calculate(cls, Scatter, idust, iscat, xprof, haze_params):
        Scatter.makephase(idust, iscat, xprof)


class ProfileModel:
    n_state_vector_entries = 30

    @classmethod
    def calculate(cls, atm, ipar, xprof):
        return atm


def _stand_in(sc, NX, ngeom, W=4):
    """a forward model whose host stage does nothing but the aerosol part of subprofretg: the Mie integration and the fit of
    the state in Variables.XN, through the module attributes as the class method reaches them"""
    from types import SimpleNamespace as NS
    from archnemesis_dist_amd.jacobian_dropin import JacobianGPU

    class StandIn(JacobianGPU):
        ansfm_device = 0
        _ansfm_staged_supported = lambda self, info: True
        check_gas_spec_atm = check_wave_range_consistency = lambda self: None
        _ansfm_thermal_inputs = lambda self: dict(alone=np.zeros((W, 1)))
        _ansfm_run_batches = lambda self, eng, recs, W: ([np.zeros((W, 1)) for _ in recs], 0, 0)
        _ansfm_convolve = lambda self, SPEC, IGEOM, disc=False: np.zeros(1)
        subspecret = lambda self, SPECONV, dS: (SPECONV, dS)

        def _ansfm_stage_one(self, IGEOM, IAV):
            x = np.asarray(self.Variables.XN, dtype=np.float64)
            theta = np.array([0.0, 90.0])
            out = sc.makephase(np.array([1.0]), 2, np.array([x[0], 0.4, 0.0]), np.array(RS), np.array([[1.4, x[1:].sum()]]), theta)
            self.fits.append(sc.subfithgm(out[2], out[3]))
            self.PathX = NS(NPATH=1)

    fm = StandIn()
    fm.fits = []
    fm.Measurement = NS(NGEOM=ngeom, NY=ngeom, NAV=np.ones(ngeom, dtype=int), NCONV=np.ones(ngeom, dtype=int), MEAS=np.zeros((1, ngeom)),
                        WGEOM=np.ones((ngeom, 1)), build_ils=lambda IGEOM: None, calc_wave_range=lambda apply_doppler, IGEOM: (0.0, 1.0))
    fm.Variables = NS(NX=NX, XN=None, models=[ProfileModel(), AerosolModel()])
    fm.Spectroscopy = NS(NGAS=0, NWAVE=W)
    return fm


class CheapDouble:
    """counts, and answers with something that depends on every argument"""
    def __init__(self):
        self.mie_calls = self.calls = 0

    def mie_makephase(self, wavel, iscat, dsize, rs, refindx, theta, radius_block=None, return_counts=False):
        self.mie_calls += 1
        v = float(dsize[0] + 3.0 * refindx[0, 1])
        return np.array([v]), np.array([2.0 * v]), np.array([0.0, 90.0, 180.0]), np.array([[3.0 + v, 1.0, 0.5 + v]])

    def hg_fit(self, theta, phase, return_counts=False):
        self.calls += 1
        return tuple(np.array([float(phase[0, 0]) * k]) for k in (1.0, 2.0, 3.0, 4.0))


def test_memo_capacity_of_a_staged_route(hooked, monkeypatch):
    sc, fmod = hooked["sc"], hooked["fmod"]
    double = CheapDouble()
    monkeypatch.setattr(fmod, "get_engine", lambda device=0: double)
    fmod.install_gpu_mie(0); fmod.install_gpu_hg_fit(0)            # fresh memos on the counting double
    fmod.set_strict(True)
    NX = 11
    x0 = np.array([0.3] + [0.001 * (j + 1) for j in range(NX - 1)])
    xnx = np.tile(x0[:, None], (1, NX + 1))
    for j in range(NX):
        xnx[j, j + 1] *= 1.05                                       # 12 distinct aerosol states
    fm = _stand_in(sc, NX, ngeom=2)
    assert fmod.aerosol_memo_capacity(fm.Variables) == 12           # 1 + the 11 elements of the model that calls makephase
    info = {}
    Y = fm._ansfm_staged_route(xnx, np.arange(NX + 1, dtype="int32"), info)
    assert Y.shape == (2, NX + 1) and len(fm.fits) == 24
    assert (double.mie_calls, double.calls) == (12, 12), (double.mie_calls, double.calls)
    assert fmod.ROUTES == {"mie": 12, "mie (memo)": 12, "hg fit": 12, "hg fit (memo)": 12}
    for k in range(12):                                             # the second geometry got the first one's results
        assert all(np.array_equal(a, b) for a, b in zip(fm.fits[k], fm.fits[12 + k]))
    assert len(set(float(f[0][0]) for f in fm.fits[:12])) == 12
    # ... and the capacity is 8 again afterwards: the same walk over 12 other states outside a route recomputes every state
    # for every geometry, as an 8-entry memo that is asked for 12 states in turn does
    assert (fmod.MIE_MEMO_ENTRIES, fmod.HG_FIT_MEMO_ENTRIES) == (8, 8)
    double.mie_calls = double.calls = 0
    for _ in range(2):
        for col in range(NX + 1):
            fm.Variables.XN = 1.01 * xnx[:, col]
            fm._ansfm_stage_one(0, 0)
    assert (double.mie_calls, double.calls) == (24, 24)
    # an exception inside a route restores the capacity too
    fm._ansfm_thermal_inputs = lambda: 1 / 0
    with pytest.raises(ZeroDivisionError):
        fm._ansfm_staged_route(xnx, np.arange(NX + 1, dtype="int32"), {})
    assert (fmod.MIE_MEMO_ENTRIES, fmod.HG_FIT_MEMO_ENTRIES) == (8, 8)
    assert "raised_memo_capacity" in inspect.getsource(importlib.import_module("archnemesis_dist_amd.jacobian_dropin")._with_aerosol_memos)
    from archnemesis_dist_amd.jacobian_dropin import JacobianGPU
    assert hasattr(JacobianGPU._ansfm_staged_limb_route, "__wrapped__") and hasattr(JacobianGPU._ansfm_staged_route, "__wrapped__")
