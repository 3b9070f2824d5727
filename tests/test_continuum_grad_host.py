"""profile_state.BatchedCKThermalModel.jacobian_analytic(sources=True) without a GPU: what it hands to the engine's fused
gradient entry (cirsradg_ck_thermal_cont) -- the mixing ratios PP / PRESS, NPAR = NVMR + 2 + NDUST, IRAY as the Rayleigh mode, f4
for IRAY 4 only, the gradients left on the device, no shared gas gradient -- the refusal of extra_continuum with sources, the
unchanged default, and the two new symbols in the prototypes read from include/ansfm.h.  The engine is a stand-in that records
calls."""
import os
import re

import numpy as np
import pytest

NPRO, NVMR, NLAY, NDUST, W, S = 12, 6, 5, 2, 7, 4


class RecordingEngine:
    """what jacobian_analytic asks of an engine, on the CPU: layers from a seeded generator, spectra of ones"""
    device = 0

    def __init__(self):
        self.calls = []
        self.WAVE = 400.0 + 10.0 * np.arange(W)

    def ktable_info(self):
        return (W, 4, 3, 3, S), None

    def layer_averageg(self, RADIUS, H, P, T, ID, VMR, DUST, PARAH2, BASEH, BASEP=None, **k):
        self.calls.append(("layer_averageg", None))
        L = BASEH.shape[0]
        nd = 0 if DUST is None else np.shape(DUST)[1]
        rng = np.random.default_rng(17)
        u = lambda *shape: rng.uniform(0.5, 1.5, shape)
        PRESS = 1.0e5 * u(L)
        out = dict(HEIGHT=BASEH.copy(), PRESS=PRESS, TEMP=150.0 * u(L), TOTAM=1.0e27 * u(L), AMOUNT=1.0e24 * u(L, NVMR),
                   PP=PRESS[:, None] * u(L, NVMR) / NVMR, CONT=1.0e9 * u(L, nd), FRAC=0.3 * u(L), DELH=2.0e4 * u(L), BASET=150.0 * u(L),
                   LAYSF=u(L), DTE=u(L, NPRO), DAM=u(L, NPRO), DCO=u(L, NPRO), DPH=u(L, NPRO))
        self.layers = out
        return tuple(out[k] for k in ("HEIGHT", "PRESS", "TEMP", "TOTAM", "AMOUNT", "PP", "CONT", "FRAC", "DELH", "BASET", "LAYSF",
                                      "DTE", "DAM", "DCO", "DPH"))

    @staticmethod
    def rayleigh_f4(ID, ISO, VMR):
        from archnemesis_dist_amd.engine import AnsfmEngine
        return AnsfmEngine.rayleigh_f4(ID, ISO, VMR)

    def upload_cia(self, ISPACE, WAVEC, *a, **k):
        self.calls.append(("upload_cia", dict(ISPACE=ISPACE)))

    def upload_dust(self, SWAVE, KEXT, KSCA=None):
        self.calls.append(("upload_dust", dict(KEXT=KEXT)))

    def set_gradient_gases(self, gases, temperature=True):
        self.calls.append(("set_gradient_gases", gases))

    def calc_tau_rayleigh(self, IRAY, ISPACE, WAVEC, TOTAM, **k):
        self.calls.append(("calc_tau_rayleigh", None))
        return np.zeros((W, TOTAM.size)), np.zeros((W, TOTAM.size))

    def cirsradg_ck_thermal(self, ISPACE, lp, lt, am, taucont, dtaucon, NVMR_, NPAR, igas_map, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF,
                            **kw):
        self.calls.append(("cirsradg_ck_thermal", dict(taucont=taucont, dtaucon=dtaucon, NPAR=NPAR, kw=kw)))
        return np.ones((W, np.atleast_1d(NLAYIN).size)), None, None

    def cirsradg_ck_thermal_cont(self, ISPACE, lp, lt, am, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, NVMR_, NPAR, igas_map, NLAYIN, LAYINC,
                                 SCALE, EMTEMP, TSURF, **kw):
        self.calls.append(("cirsradg_ck_thermal_cont", dict(ISPACE=ISPACE, lp=lp, lt=lt, am=am, q=q, FRAC=FRAC, TOTAM=TOTAM, DELH=DELH,
                                                            CONT=CONT, IRAY=IRAY, f4=f4, NVMR=NVMR_, NPAR=NPAR, igas_map=igas_map,
                                                            TSURF=TSURF, kw=kw)))
        return np.ones((W, np.atleast_1d(NLAYIN).size)), None, None

    def map2pro(self, dSPECIN, *a, **kw):
        self.calls.append(("map2pro", dict(dSPECIN=dSPECIN, kw=kw)))

    def map2xvec(self, dSPECIN, NWAVE, NVMR_, NDUST_, NPRO_, NPATH, NX, xmap):
        self.calls.append(("map2xvec", dict(dSPECIN=dSPECIN, NDUST=NDUST_)))
        return np.zeros((NWAVE, NPATH, NX))


def model(eng, IRAY, cia=True, dust=True, extra=None):
    from archnemesis_dist_amd import synthetic as syn
    from archnemesis_dist_amd.profile_state import ContinuousProfileState, BatchedCKThermalModel
    pr = syn.synth_profiles(NPRO, NVMR, seed=9)
    st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("VMR", 1)])
    ciad = dict(CIA_WAVEN=np.linspace(0.0, 2000.0, 9), CIA_TEMP=np.array([50.0, 150.0, 400.0]), CIA_FRAC=np.array([0.0]), NPARA=0,
                K_CIA=np.ones((2, 1, 3, 9)), IPAIRG1=[39, 39], IPAIRG2=[39, 40], INORMALT=[0, 0], INORMAL=0, INORMALD=[False, False])
    dustd = dict(SWAVE=np.array([300.0, 400.0, 500.0, 600.0]), KEXT=np.ones((4, NDUST)), KSCA=0.5 * np.ones((4, NDUST)),
                 DUST=np.full((NPRO, NDUST), 1.0e3))
    m = BatchedCKThermalModel(eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], [2, 3, 4, 5], layering_args=dict(NLAY=NLAY), IRAY=IRAY,
                              cia=ciad if cia else None, dust=dustd if dust else None, extra_continuum=extra)
    return m, st, pr


@pytest.mark.parametrize("IRAY", [0, 1, 4])
def test_sources_route_hands_the_layer_arrays_to_the_fused_gradient_entry(IRAY):
    eng = RecordingEngine()
    m, st, pr = model(eng, IRAY)
    YN, KK = m.jacobian_analytic(sources=True)
    assert YN.shape == (W,) and KK.shape == (W, st.NX)
    names = [name for name, _ in eng.calls]
    assert names == ["layer_averageg", "upload_cia", "upload_dust", "set_gradient_gases", "cirsradg_ck_thermal_cont", "map2pro",
                     "set_gradient_gases", "map2xvec"]
    rec = dict(eng.calls)
    lay, c = eng.layers, rec["cirsradg_ck_thermal_cont"]
    q = lay["PP"] / lay["PRESS"][:, None]
    assert np.array_equal(c["q"], q)
    for k in ("FRAC", "TOTAM", "DELH", "CONT"):
        assert np.array_equal(c[k], lay[k]), k
    assert np.array_equal(c["lp"], lay["PRESS"]) and np.array_equal(c["lt"], lay["TEMP"])
    assert np.array_equal(c["am"], np.ascontiguousarray(lay["AMOUNT"][:, [2, 3, 4, 5]].T) * 1.0e-4)
    assert (c["ISPACE"], c["NVMR"], c["NPAR"], c["IRAY"]) == (0, NVMR, NVMR + 2 + NDUST, IRAY)
    assert np.array_equal(c["igas_map"], [2, 3, 4, 5])
    if IRAY == 4:
        f4 = np.zeros((NLAY, 4)); f4[:, 0] = q[:, 0]; f4[:, 1] = q[:, 1]; f4[:, 2] = q[:, 2]; f4[:, 3] = q[:, 3]
        assert np.array_equal(c["f4"], f4)                 # ID 39, 40, 6, 11 are the first four gases
    else:
        assert c["f4"] is None
    assert c["kw"] == dict(gradients_on_device=True)       # no dtau_every_gas: the Rayleigh term is in the dense gradients
    assert rec["map2pro"]["dSPECIN"] is None and rec["map2pro"]["kw"] == dict(to_host=False)
    assert rec["map2xvec"]["dSPECIN"] is None and rec["map2xvec"]["NDUST"] == NDUST
    assert "calc_tau_rayleigh" not in names and "cirsradg_ck_thermal" not in names
    # a second call does not upload the sources again
    del eng.calls[:]
    m.jacobian_analytic(sources=True)
    assert [name for name, _ in eng.calls][:3] == ["layer_averageg", "set_gradient_gases", "cirsradg_ck_thermal_cont"]


@pytest.mark.parametrize("cia,dust", [(True, False), (False, True)])
def test_a_source_that_is_absent_is_switched_off(cia, dust):
    eng = RecordingEngine()
    m, st, pr = model(eng, 1, cia=cia, dust=dust)
    m.jacobian_analytic(sources=True)
    c = dict(eng.calls)["cirsradg_ck_thermal_cont"]
    nd = NDUST if dust else 0
    assert c["NPAR"] == NVMR + 2 + nd and c["TOTAM"] is not None
    assert (c["q"] is not None, c["FRAC"] is not None, c["DELH"] is not None, c["CONT"] is not None) == (cia, cia, cia, dust)
    assert ("upload_cia" in dict(eng.calls), "upload_dust" in dict(eng.calls)) == (cia, dust)


def test_extra_continuum_with_sources_is_refused():
    eng = RecordingEngine()
    m, st, pr = model(eng, 1, extra=np.zeros((W, NLAY)))
    with pytest.raises(NotImplementedError, match="extra_continuum"):
        m.jacobian_analytic(sources=True)
    assert eng.calls == []


def test_default_is_unchanged():
    eng = RecordingEngine()
    m, st, pr = model(eng, 1)
    with pytest.raises(NotImplementedError, match="sources=True"):
        m.jacobian_analytic()
    with pytest.raises(NotImplementedError, match="sources=True"):
        m.jacobian_analytic(st.XN)
    assert eng.calls == []
    # a model without sources takes the route it always took, with or without the keyword
    for kw in (dict(), dict(sources=True)):
        eng = RecordingEngine()
        m, st, pr = model(eng, 1, cia=False, dust=False)
        m.jacobian_analytic(**kw)
        names = [name for name, _ in eng.calls]
        assert names == ["layer_averageg", "calc_tau_rayleigh", "set_gradient_gases", "cirsradg_ck_thermal", "map2pro",
                         "set_gradient_gases", "map2xvec"]
        c = dict(eng.calls)["cirsradg_ck_thermal"]
        assert c["dtaucon"] is None and set(c["kw"]) == {"gradients_on_device", "dtau_every_gas"}


def test_the_two_entries_are_in_the_prototypes_read_from_the_header():
    import ctypes as C
    from archnemesis_dist_amd import _lib
    header = open(os.path.join(_lib.INCLUDE, "ansfm.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name in ("ansfm_cirsradg_ck_thermal_cont", "ansfm_cirsradg_ck_thermal_cont_dev"):
        assert name in _lib.PROTOTYPES and name in _lib.EXPORTS
        decl = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, text).group(1)
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == len(decl.split(",")) == 31
        # the arguments of ansfm_cirsradg_ck_thermal without taucont / dtaucon, with the nine of the continuum block
        assert len(argtypes) == len(_lib.PROTOTYPES["ansfm_cirsradg_ck_thermal"][1]) - 2 + 9
        by_value = [i for i, t in enumerate(argtypes) if t is C.c_int]
        assert by_value == [1, 2, 3, 7, 12, 14, 16, 17, 19, 20]   # ISPACE n L use_cia use_dust ray_mode NVMR NPAR P LIMAX
        assert all(t is C.c_void_p for i, t in enumerate(argtypes) if i not in by_value)
