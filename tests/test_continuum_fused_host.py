"""profile_dropin.ReferenceProfileBatch and the fused continuum entry, without a GPU: with an engine that has
cirsrad_ck_thermal_cont_dev the CIA table and the aerosol cross sections are uploaded once per geometry and the entry
receives the per-state layer arrays; with an engine that lacks it the call sequence is the one through calc_tau_cia /
calc_tau_dust and a dense taucont.  The forward model and the engine are stand-ins that record calls."""
import types

import numpy as np
import pytest

NPRO, NVMR, NLAY, NDUST, W = 12, 6, 5, 2, 7


class RecordingEngine:
    """what ReferenceProfileBatch asks of an engine, on the CPU: layers from a seeded generator, spectra of ones"""
    device = 0

    def __init__(self):
        self.calls = []

    @property
    def torch_device(self):
        import torch
        return torch.device("cpu")

    def layer_average(self, RADIUS, H, P, T, ID, VMR, DUST, PARAH2, BASEH, BASEP=None, **k):
        self.calls.append(("layer_average", None))
        n, L = BASEH.shape
        rng = np.random.default_rng(17)
        u = lambda *shape: rng.uniform(0.5, 1.5, shape)
        PRESS = 1.0e5 * u(n, L)
        out = dict(HEIGHT=BASEH.copy(), PRESS=PRESS, TEMP=150.0 * u(n, L), TOTAM=1.0e27 * u(n, L), AMOUNT=1.0e24 * u(n, L, NVMR),
                   PP=PRESS[:, :, None] * u(n, L, NVMR) / NVMR, CONT=1.0e9 * u(n, L, DUST.shape[2]), FRAC=0.3 * u(n, L),
                   DELH=2.0e4 * u(n, L), BASET=150.0 * u(n, L), LAYSF=u(n, L))
        self.layers = out
        return tuple(out[k] for k in ("HEIGHT", "PRESS", "TEMP", "TOTAM", "AMOUNT", "PP", "CONT", "FRAC", "DELH", "BASET", "LAYSF"))

    @staticmethod
    def rayleigh_f4(ID, ISO, VMR):
        from archnemesis_dist_amd.engine import AnsfmEngine
        return AnsfmEngine.rayleigh_f4(ID, ISO, VMR)

    def calc_tau_cia(self, ISPACE, WAVEC, *a, **k):
        self.calls.append(("calc_tau_cia", None))
        return np.zeros((np.size(WAVEC), a[12].shape[0]))                # PP is the 13th argument after WAVEC

    def calc_tau_dust(self, WAVEC, SWAVE, KEXT, KSCA, CONT):
        self.calls.append(("calc_tau_dust", None))
        return tuple(np.zeros((np.size(WAVEC), CONT.shape[0], CONT.shape[1])) for _ in range(4))

    def calc_tau_rayleigh_batch_dev(self, IRAY, ISPACE, TOTAM, out, ID=None, ISO=None, VMR=None, variant=None):
        self.calls.append(("calc_tau_rayleigh_batch_dev", None))
        out.zero_()
        return out

    def cirsrad_ck_thermal_dev(self, ISPACE, n, L, lp, lt, am, cont, *rest):
        self.calls.append(("cirsrad_ck_thermal_dev", dict(cont=cont)))
        rest[-1].fill_(1.0)

    def last_layer_rows(self):
        return (1, 1)

    def synchronize(self):
        pass


class FusedRecordingEngine(RecordingEngine):
    def upload_cia(self, ISPACE, WAVEC, *a, **k):
        self.calls.append(("upload_cia", dict(ISPACE=ISPACE, WAVEC=np.array(WAVEC), args=a, kw=k)))

    def upload_dust(self, SWAVE, KEXT, KSCA=None):
        self.calls.append(("upload_dust", dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA)))

    def clear_continuum_sources(self):
        self.calls.append(("clear_continuum_sources", None))

    def cirsrad_ck_thermal_cont_dev(self, ISPACE, n, L, lp, lt, am, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, *rest):
        self.calls.append(("cirsrad_ck_thermal_cont_dev", dict(ISPACE=ISPACE, n=n, L=L, q=q, FRAC=FRAC, TOTAM=TOTAM, DELH=DELH,
                                                               CONT=CONT, IRAY=IRAY, f4=f4, rest=rest)))
        rest[-1].fill_(1.0)


class RefusingEngine(FusedRecordingEngine):
    def upload_cia(self, *a, **k):
        self.calls.append(("upload_cia", None))
        raise NotImplementedError("a para-H2 table whose bracket could leave K_CIA")


def forward_model(monkeypatch, engine):
    """the attributes of a ForwardModel_0 that ReferenceProfileBatch reads, for a nadir thermal-emission run with CIA and
    two aerosol populations, the first renormalised"""
    from archnemesis_dist_amd import synthetic as syn, layering, forward_model as fmod
    ns = types.SimpleNamespace
    pr = syn.synth_profiles(NPRO, NVMR, seed=9)
    WAVE = 400.0 + 10.0 * np.arange(W)
    A = ns(NP=NPRO, NVMR=NVMR, P=pr["P"], T=pr["T"], VMR=pr["VMR"], H=pr["H"], MOLWT=np.full(NPRO, 2.3e-3), ID=pr["ID"],
           ISO=pr["ISO"], DUST=np.full((NPRO, NDUST), 1.0e3), PARAH2=None, DUST_UNITS_FLAG=None, DUST_RENORMALISATION={0: 2.5},
           locate_gas=lambda gid, iso: int(np.nonzero(pr["ID"] == gid)[0][0]), NLOCATIONS=1)
    spec = ns(WAVE=WAVE, NGAS=2, ID=[6, 11], ISO=[0, 0], read_tables=lambda wavemin, wavemax: None)
    CIA = ns(WAVEN=np.linspace(0.0, 2000.0, 9), TEMP=np.array([50.0, 150.0, 400.0]), FRAC=np.array([0.0]), NPARA=0,
             K_CIA=np.ones((2, 1, 3, 9)), IPAIRG1=[39, 39], IPAIRG2=[39, 40], INORMALT=[0, 0], INORMAL=0,
             locate_INORMAL_pairs=lambda: np.array([False, False]))
    M = ns(NGEOM=1, NAV=[1], WGEOM=np.ones((1, 1)), EMISS_ANG=np.array([[15.0]]), TANHE=np.zeros((1, 1)), ISPACE=0,
           build_ils=lambda IGEOM: None, calc_wave_range=lambda apply_doppler, IGEOM: (WAVE[0], WAVE[-1]))
    fm = ns(Atmosphere=A, Spectroscopy=spec, CIA=CIA, Measurement=M, Variables=ns(LX=np.zeros(NPRO, dtype=int)),
            Scatter=ns(NDUST=NDUST, IRAY=4, WAVE=np.array([300.0, 400.0, 500.0, 600.0]), KEXT=np.ones((4, NDUST)),
                       KSCA=0.5 * np.ones((4, NDUST))),
            Surface=ns(TSURF=-1.0), Layer=ns(RADIUS=pr["RADIUS"], NLAY=NLAY, LAYTYP=layering.EQUAL_LOG_PRESSURE, LAYINT=1, NINT=101,
                                              LAYHT=0.0),
            adjust_hydrostat=False, ansfm_device=0, check_gas_spec_atm=lambda: None, check_wave_range_consistency=lambda: None,
            _ansfm_upload_table=lambda eng: eng.calls.append(("upload_table", None)))
    monkeypatch.setattr(fmod, "get_engine", lambda device=0: engine)
    return fm, pr


def run(monkeypatch, engine, n=3):
    from archnemesis_dist_amd.profile_dropin import ReferenceProfileBatch
    fm, pr = forward_model(monkeypatch, engine)
    batch = ReferenceProfileBatch(fm, [("T", None, "profile", 0, NPRO)])
    X = np.repeat(pr["T"][None], n, 0) * (1.0 + 0.01 * np.arange(n)[:, None])
    Y = batch.spectra_batch(X)
    assert tuple(Y.shape) == (n, W)
    return fm, [name for name, _ in engine.calls], dict((name, rec) for name, rec in engine.calls)


def test_fused_entry_receives_the_layer_arrays_of_every_state(monkeypatch):
    eng = FusedRecordingEngine()
    fm, names, rec = run(monkeypatch, eng)
    assert names == ["upload_table", "upload_cia", "upload_dust", "layer_average", "cirsrad_ck_thermal_cont_dev"]
    up = rec["upload_cia"]
    assert up["ISPACE"] == 0 and np.array_equal(up["WAVEC"], fm.Spectroscopy.WAVE) and np.array_equal(up["args"][0], fm.CIA.WAVEN)
    assert up["kw"] == dict(k_co2=None, k_n2n2=None, k_n2h2=None)
    assert np.array_equal(rec["upload_dust"]["KEXT"], fm.Scatter.KEXT) and np.array_equal(rec["upload_dust"]["KSCA"], fm.Scatter.KSCA)
    lay, c = eng.layers, rec["cirsrad_ck_thermal_cont_dev"]
    assert (c["ISPACE"], c["n"], c["L"], c["IRAY"]) == (0, 3, NLAY, 4)
    num = lambda t: t.cpu().numpy()
    q = lay["PP"] / lay["PRESS"][:, :, None]
    assert np.array_equal(num(c["q"]), q)
    for k in ("FRAC", "TOTAM", "DELH"):
        assert np.array_equal(num(c[k]), lay[k]), k
    CONT = lay["CONT"].copy()                            # calc_tau_dust's renormalisation of the first population (:4833)
    CONT[:, :, 0] = CONT[:, :, 0] / CONT[:, :, 0].sum(axis=1, keepdims=True) * 1e4 * 2.5
    assert np.array_equal(num(c["CONT"]), CONT) and not np.array_equal(CONT, lay["CONT"])
    f4 = np.zeros((3, NLAY, 4)); f4[..., 0] = q[..., 0]; f4[..., 1] = q[..., 1]; f4[..., 2] = q[..., 2]; f4[..., 3] = q[..., 3]
    assert np.array_equal(num(c["f4"]), f4)              # ID 39, 40, 6, 11 are the first four gases
    assert "calc_tau_cia" not in names and "calc_tau_dust" not in names


def test_engine_without_the_entry_keeps_the_dense_route(monkeypatch):
    _, names, rec = run(monkeypatch, RecordingEngine())
    assert names == ["upload_table", "layer_average", "calc_tau_cia", "calc_tau_dust", "calc_tau_rayleigh_batch_dev",
                     "cirsrad_ck_thermal_dev"]
    assert tuple(rec["cirsrad_ck_thermal_dev"]["cont"].shape) == (3, W, NLAY)


def test_refused_source_keeps_the_dense_route(monkeypatch):
    _, names, _ = run(monkeypatch, RefusingEngine())
    assert names == ["upload_table", "upload_cia", "clear_continuum_sources", "layer_average", "calc_tau_cia", "calc_tau_dust",
                     "calc_tau_rayleigh_batch_dev", "cirsrad_ck_thermal_dev"]
