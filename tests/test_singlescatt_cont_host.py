"""What the single-scattering batch with its continuum formed on the device needs off the device: the entry
ansfm_cirsrad_ck_singlescatt_batch_cont in the header, the library and the engine; the refusals of
scatter_state.BatchedCKSingleScatterModel and what its spectra_batch hands to the engine; and, against the reference itself, the
NumPy restatement of the scattering opacity and the layer-mean phase function that the GPU tests compare with."""
import importlib.util
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_import import REFERENCE_ROOT as REF  # noqa: E402
ENTRY = "ansfm_cirsrad_ck_singlescatt_batch_cont"
BLOCK = ["int use_cia", "const double *lay_q", "const double *lay_frac", "const double *lay_totam", "const double *lay_delh",
         "int use_dust", "const double *lay_cont", "int ray_mode", "const double *f4"]


def _header_args(name):
    with open(os.path.join(ROOT, "include", "ansfm.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    m = re.search(r"\bint " + name + r"\s*\(([^()]*)\)\s*;", text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_is_declared_exported_and_bound():
    import ctypes as C
    import archnemesis_dist_amd as pkg
    from archnemesis_dist_amd import _lib
    args = _header_args(ENTRY)
    assert ENTRY in _lib.EXPORTS
    restype, argtypes = _lib.PROTOTYPES[ENTRY]
    assert restype is C.c_int and len(argtypes) == len(args)
    # the dense batch entry's arguments without taucont, tausca and phase, plus the continuum block of the thermal entry, ncont
    # and phase_fn
    dense = _header_args("ansfm_cirsrad_ck_singlescatt_batch")
    gone = {"const double *taucont", "const double *tausca", "const double *phase"}
    kept = [a for a in dense if a not in gone]
    assert len(kept) == len(dense) - 3
    i = args.index("int use_cia")
    assert args[:i] == kept[:i] and args[i:i + len(BLOCK)] == BLOCK
    assert args[i + len(BLOCK):i + len(BLOCK) + 2] == ["int ncont", "const double *phase_fn"] and args[i + len(BLOCK) + 2:] == kept[i:]
    thermal = _header_args("ansfm_cirsrad_ck_thermal_cont_dev")
    j = thermal.index("int use_cia")
    assert thermal[j:j + len(BLOCK)] == BLOCK
    for a, t in zip(args, argtypes):
        assert t is (C.c_void_p if "*" in a else C.c_int), a
    assert hasattr(_lib.load(), ENTRY)                          # the library exports it
    fn = pkg.AnsfmEngine.cirsrad_ck_singlescatt_batch_cont
    assert list(inspect.signature(fn).parameters)[:14] == ["self", "ISPACE", "lay_press_pa", "lay_temp", "amount", "q", "FRAC", "TOTAM",
                                                           "DELH", "CONT", "IRAY", "f4", "phase_fn", "NLAYIN"]
    assert _lib.load().ansfm_abi_version() == 1


def _profiles(NPRO=7, NVMR=3, NDUST=2, seed=2):
    rng = np.random.default_rng(seed)
    H = np.linspace(0.0, 6.0e4, NPRO); P = 1.0e5 * np.exp(-H / 1.0e4); T = rng.uniform(100.0, 200.0, NPRO)
    VMR = rng.uniform(1e-6, 1e-2, (NPRO, NVMR)); DUST = rng.uniform(1.0, 1.0e3, (NPRO, NDUST))
    return H, P, T, VMR, DUST


class RecordingEngine:
    """what BatchedCKSingleScatterModel asks of an engine, without a device: records every call"""
    device = 0

    def __init__(self, W, S):
        self.W, self.S, self.calls = W, S, []
        self.WAVE = 100.0 + 20.0 * np.arange(W)

    def ktable_info(self):
        return (self.W, 4, 8, 6, self.S), True

    def layer_average(self, RADIUS, H, P, T, ID, VMR, DUST, PARAH2, BASEH, BASEP, **kw):
        self.calls.append(("layer_average", None))
        n, L, NVMR = T.shape[0], BASEH.size, VMR.shape[2]
        ND = 0 if DUST is None else DUST.shape[2]
        lin = lambda lo, hi: np.repeat(np.linspace(lo, hi, L)[None], n, 0)
        TEMP = lin(200.0, 120.0) + T.mean(1)[:, None] * 1e-3
        return (lin(0.0, 5.0e4), lin(1.0e5, 1.0e2), TEMP, lin(1e27, 1e24), np.ones((n, L, NVMR)) * 1e24,
                np.ones((n, L, NVMR)) * 10.0, np.ones((n, L, ND)) * 1e9, np.full((n, L), 0.25), lin(4.0e3, 6.0e3), TEMP, np.ones((n, L)))

    def upload_cia(self, *a, **kw):
        self.calls.append(("upload_cia", None))

    def upload_dust(self, *a, **kw):
        self.calls.append(("upload_dust", None))

    def cirsrad_ck_singlescatt_batch_cont(self, *a, **kw):
        self.calls.append(("fused", (a, kw)))
        n = np.shape(a[1])[0]
        return np.zeros((n, self.W, np.shape(a[11])[1]))

    def last_layer_rows(self):
        return (0, 0)

    def last_rt_shared(self):
        return False


def _model(eng, st, W, ND, **kw):
    from archnemesis_dist_amd.scatter_state import BatchedCKSingleScatterModel
    args = dict(layering_args=dict(NLAY=5), IRAY=1)
    args.update(kw)
    return BatchedCKSingleScatterModel(eng, st, 7.0e7, [39, 40, 6], [0, 0, 0], [2], np.ones((W, 1, ND + 1)), [30.0], [20.0], np.ones(W), **args)


def test_model_refusals_need_no_device():
    from archnemesis_dist_amd.profile_state import ContinuousProfileState
    H, P, T, VMR, _ = _profiles()
    NPRO = H.size
    eng = RecordingEngine(5, 1)
    D8 = np.ones((NPRO, 8))
    K8 = dict(SWAVE=np.linspace(1.0, 2.0, 4), KEXT=np.ones((4, 8)), KSCA=np.ones((4, 8)))
    with pytest.raises(NotImplementedError, match="7"):
        _model(eng, ContinuousProfileState(H, P, T, VMR, ["T", ("DUST", 0)], DUST=D8), 5, 8, dust=K8)
    with pytest.raises(NotImplementedError, match="7"):
        _model(eng, ContinuousProfileState(H, P, T, VMR, ["T"]), 5, 8, dust=dict(K8, DUST=D8))
    D2 = np.ones((NPRO, 2))
    K2 = dict(SWAVE=np.linspace(1.0, 2.0, 4), KEXT=np.ones((4, 2)), KSCA=np.ones((4, 2)))
    with pytest.raises(NotImplementedError, match="DUST_RENORMALISATION"):
        _model(eng, ContinuousProfileState(H, P, T, VMR, ["T", ("DUST", 0)], DUST=D2), 5, 2, dust=K2, DUST_RENORMALISATION=True)
    with pytest.raises(ValueError):                             # a DUST block without the cross sections
        _model(eng, ContinuousProfileState(H, P, T, VMR, ["T", ("DUST", 0)], DUST=D2), 5, 2)
    with pytest.raises(ValueError):                             # cross sections of three populations, profiles of two
        _model(eng, ContinuousProfileState(H, P, T, VMR, ["T", ("DUST", 0)], DUST=D2), 5, 2,
               dust=dict(K2, KEXT=np.ones((4, 3)), KSCA=np.ones((4, 3))))
    with pytest.raises(ValueError):                             # neither aerosols nor Rayleigh: nothing scatters
        _model(eng, ContinuousProfileState(H, P, T, VMR, ["T"]), 5, 0, IRAY=0)
    with pytest.raises(ValueError):                             # phase_fn of one population, two in the state
        _model(eng, ContinuousProfileState(H, P, T, VMR, ["T", ("DUST", 0)], DUST=D2), 5, 1, dust=K2)
    assert not eng.calls


def test_spectra_batch_hands_over_layers_not_spectral_arrays():
    """the fused route: one call of the fused entry with (n, L, ...) arrays and nothing of shape (n, W, L)"""
    from archnemesis_dist_amd.profile_state import ContinuousProfileState
    H, P, T, VMR, DUST = _profiles()
    NPRO, W, NLAY = H.size, 9, 5
    st = ContinuousProfileState(H, P, T, VMR, ["T", ("VMR", 1), ("DUST", 1)], DUST=DUST)
    eng = RecordingEngine(W, 1)
    K2 = dict(SWAVE=np.linspace(50.0, 400.0, 4), KEXT=np.ones((4, 2)), KSCA=np.ones((4, 2)))
    cia = dict.fromkeys(("CIA_WAVEN", "CIA_TEMP", "CIA_FRAC", "NPARA", "K_CIA", "IPAIRG1", "IPAIRG2", "INORMALT", "INORMAL", "INORMALD"))
    model = _model(eng, st, W, 2, dust=K2, cia=cia, layering_args=dict(NLAY=NLAY))
    assert model.fused_continuum is True and model.ny() == W and model.state is st
    n = 4
    X = np.repeat(st.XN[None], n, 0)
    X[1, 2] += 1.0; X[2, NPRO + 3] += 0.05; X[3, 2 * NPRO + 1] += 0.05
    model.spectra_batch(X, device="cpu")
    names = [k for k, _ in eng.calls]
    assert names == ["layer_average", "upload_cia", "upload_dust", "fused"]
    a, kw = eng.calls[-1][1]
    ISPACE, lp, lt, am, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, phase_fn, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF = a[:17]
    assert (ISPACE, IRAY, f4) == (0, 1, None)
    assert lp.shape == lt.shape == FRAC.shape == TOTAM.shape == DELH.shape == (n, NLAY)
    assert am.shape == (n, 1, NLAY) and q.shape == (n, NLAY, 3) and CONT.shape == (n, NLAY, 2)
    assert phase_fn.shape == (W, 1, 3) and SCALE.shape == EMTEMP.shape == (n, NLAY, 1) and TSURF.shape == (n,)
    assert NLAYIN.tolist() == [NLAY] and LAYINC.shape == (NLAY, 1)
    for v in list(a) + list(kw.values()):                       # nothing per (state, wavenumber, layer)
        assert np.ndim(v) < 3 or W not in np.shape(v)[1:] or np.shape(v)[0] != n, np.shape(v)
    model.spectra_batch(X, device="cpu")                        # the sources stay resident
    assert [k for k, _ in eng.calls][4:] == ["layer_average", "fused"]


def test_restatement_equals_the_module_function():
    """the tests' restatement of :4316-4321 and scatter_state's give the same bits, negative and zero opacities included"""
    import singlescatt_cont_cases as cc
    from archnemesis_dist_amd.scatter_state import singlescatt_phase_and_sca
    rng = np.random.default_rng(5)
    for ND in (0, 2, 7):
        W, L, P = 6, 5, 3
        cl = rng.uniform(-1e-3, 1e-2, (W, L, ND)); cl[:, 2] = 0.0
        ray = rng.uniform(0.0, 1e-3, (W, L)) * (ND % 2 == 0)
        pf = rng.uniform(-0.2, 2.0, (W, P, ND + 1))
        a, b = cc.reference_sca_and_phase(cl, ray, np.sum(cl, 2), pf), singlescatt_phase_and_sca(cl, ray, np.sum(cl, 2), pf)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


@pytest.mark.needs_reference
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "archnemesis")), reason="reference tree not present")
def test_restatement_reproduces_what_the_reference_layer_loop_read():
    """The case of tools/golden/gen_golden_jacobian_ss.py, one forward model: calc_singlescatt_plane_spectrum is wrapped as that
    script wraps it, and the restatement of `sca` and `phase` from LayerX.TAUCLSCAT / TAURAY / TAUSCAT and calc_phase gives, bit
    for bit, the albedo and the phase function the reference's layer loop read on every path."""
    import shutil
    import tempfile
    import singlescatt_cont_cases as cc
    from oracle.ref_import import import_reference
    from oracle import gen_golden_jacobian as gj
    spec = importlib.util.spec_from_file_location("gen_golden_jacobian_ss", os.path.join(ROOT, "tools", "golden", "gen_golden_jacobian_ss.py"))
    gss = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gss)
    ans = import_reference()
    fm_mod = sys.modules["archnemesis.ForwardModel_0"]
    work = tempfile.mkdtemp(prefix="ansfm_sscont_")
    gj.setup_c1(ans, work, seed=4, case=gss.CASE)
    o_ss, o_cirs = fm_mod.calc_singlescatt_plane_spectrum, fm_mod.ForwardModel_0.CIRSrad
    seen, checked = [], []

    def w_ss(*a):
        seen.append(tuple(np.array(x) for x in a))
        return o_ss(*a)

    def w_cirs(self, return_grad=False):
        del seen[:]
        res = o_cirs(self, return_grad)
        S, Lx, Px, Sc = self.SpectroscopyX, self.LayerX, self.PathX, self.ScatterX
        NPATH, ND = int(Px.NPATH), int(Sc.NDUST)
        assert len(seen) == NPATH
        rad = np.pi / 180.
        calpha = np.sin(Px.SOL_ANG * rad) * np.sin(Px.EMISS_ANG * rad) * np.cos(Px.AZI_ANG * rad - np.pi) - np.cos(Px.EMISS_ANG * rad) * np.cos(Px.SOL_ANG * rad)
        alpha = np.arccos(calpha) / np.pi * 180.
        phase_fn = np.zeros((S.NWAVE, NPATH, ND + 1))               # phase_function of :4269-4271 before the transpose
        phase_fn[:, :, 0:ND] = Sc.calc_phase(alpha, S.WAVE)
        phase_fn[:, :, ND] = Sc.calc_phase_ray(alpha)
        sca, phase = cc.reference_sca_and_phase(np.array(Lx.TAUCLSCAT), np.array(Lx.TAURAY), np.array(Lx.TAUSCAT), phase_fn)
        omega = np.zeros((S.NWAVE, S.NG, Lx.NLAY))
        iin = np.where(Lx.TAUTOT > 0.0)
        omega[iin[0], iin[1], iin[2]] = sca[iin[0], iin[2]] / Lx.TAUTOT[iin[0], iin[1], iin[2]]
        for ip in range(NPATH):
            n = int(Px.NLAYIN[ip])
            li = Px.LAYINC[:n, ip]
            assert np.array_equal(phase[ip][:, li], seen[ip][5]) and np.array_equal(omega[:, :, li], seen[ip][4])
            assert np.any(seen[ip][5] > 0) and np.any(seen[ip][4] > 0)
            checked.append(ip)
        return res

    cwd = os.getcwd()
    os.chdir(work)
    try:
        fm_mod.calc_singlescatt_plane_spectrum = w_ss
        fm_mod.ForwardModel_0.CIRSrad = w_cirs
        FM = gss.cut_case(ans)
        FM.nemesisfm()
        assert checked and checked[0] == 0
    finally:
        os.chdir(cwd)
        fm_mod.calc_singlescatt_plane_spectrum = o_ss
        fm_mod.ForwardModel_0.CIRSrad = o_cirs
        shutil.rmtree(work, ignore_errors=True)
