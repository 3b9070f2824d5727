"""What AnsfmEngine's host-array wrappers hand to the library, without a GPU and without libansfm.so.

The engine is made with object.__new__ and its `_lib` is a recorder: every `ansfm_*` attribute is a Python callable that
checks the call against the prototype read from include/ansfm.h (argument count, Python int for `int`, float for `double`,
None or c_void_p for a pointer), compares every input array byte for byte with an array the test built from the layouts
the header documents -- at call time, while the wrapper's locals are alive -- and writes a ramp into every output, so
that what the wrapper returns (shape, dropped axis, which buffer) can be checked too.

The wrappers share their marshalling (`_layer_args`, `_path_args`, `_gradient_result`, ...).  Everything here but the three
`test_difference_*` tests also held for the per-entry copies those helpers replaced, argument for argument; the three pin
what the helpers changed on purpose: NLAYIN is checked by every entry, a batch wants lay_temp (n_models, NLAY) as given
and broadcasts SCALE / EMTEMP (LIMAX, NPATH), and a failed gradient call leaves no chain to map2pro.
"""
import ctypes as C

import numpy as np
import pytest

from archnemesis_dist_amd import _lib
from archnemesis_dist_amd.engine import AnsfmEngine, _fingerprint

W, G, NPG, NTG, S = 5, 2, 4, 3, 2
L, P, LIMAX = 3, 2, 3
NPAR, NVMR, Q = 4, 2, 2
ND, NTH, NMU, NF = 2, 4, 2, 1

f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32)


class Out:
    """an output slot: `size` float64 that the recorder fills with base, base + 1, ...; null: the slot must be NULL"""

    def __init__(self, *shape, base=0.0, null=False):
        self.shape, self.base, self.null = shape, base, null

    @property
    def ramp(self):
        return self.base + np.arange(int(np.prod(self.shape)), dtype=np.float64).reshape(self.shape)


class Recorder:
    """stands in for the ctypes library: `expect()` scripts the calls that must come, in order; with script = None every
    call is recorded and answered with `rc.get(name, 0)`"""

    def __init__(self):
        self.calls, self.script, self.rc = [], [], {}

    def expect(self, name, *exp, rc=0):
        self.script.append((name, exp, rc))

    def ansfm_last_error(self, ctx):
        return b"recorded"

    def ansfm_ktable_info(self, ctx, dims, mono):
        dims[:] = [W, G, NPG, NTG, S]
        return 0

    def __getattr__(self, name):
        if not name.startswith("ansfm_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        _, argtypes = _lib.PROTOTYPES[name]
        assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)} parameters"
        for i, (a, t) in enumerate(zip(args, argtypes)):
            if t is C.c_int:
                assert isinstance(a, int) and not isinstance(a, bool), f"{name}: argument {i} is {type(a)}, not int"
            elif t is C.c_double:
                assert isinstance(a, float), f"{name}: argument {i} is {type(a)}, not float"
            else:
                assert t is C.c_void_p and (a is None or isinstance(a, C.c_void_p)), f"{name}: argument {i} is {type(a)}"
        assert args[0].value == 1
        self.calls.append((name, args))
        if self.script is None:
            return self.rc.get(name, 0)
        assert self.script, f"unexpected call of {name}"
        exp_name, exp, rc = self.script.pop(0)
        assert name == exp_name and len(exp) == len(args) - 1, (name, exp_name, len(exp), len(args) - 1)
        for i, (a, e) in enumerate(zip(args[1:], exp), start=1):
            where = f"{name}: argument {i}"
            if e is None or (isinstance(e, Out) and e.null):
                assert a is None, where
            elif isinstance(e, Out):
                r = e.ramp
                C.memmove(a.value, r.ctypes.data, r.nbytes)
            elif isinstance(e, np.ndarray):
                assert e.flags.c_contiguous and a is not None, where
                assert C.string_at(a.value, e.nbytes) == e.tobytes(), where
            else:
                assert type(a) is type(e) and a == e, f"{where}: {a!r} != {e!r}"
        return rc


@pytest.fixture
def eng():
    e = object.__new__(AnsfmEngine)
    e._lib = Recorder()
    e._ctx = C.c_void_p(1)
    e.dims = (W, G, NPG, NTG, S)
    e.cia_nvmr, e.dust_n = NVMR, ND
    yield e
    assert not e._lib.script, "scripted calls that never came: %s" % [s[0] for s in e._lib.script]
    e._ctx = C.c_void_p()           # nothing for __del__ to destroy


def view(rng, *shape, dtype=np.float32):
    """a non-contiguous view (every other element of the last axis) of the given shape and dtype"""
    a = rng.uniform(1.0, 2.0, shape[:-1] + (2 * shape[-1],)).astype(dtype)
    return a[..., ::2]


def layers(n, axis=True, npar=NPAR, seed=1):
    """lay_press_pa, lay_temp, amount, taucont, dtaucon of n models; axis=False (n = 1): without the model axis"""
    rng = np.random.default_rng(seed)
    lead = (n,) if axis else ()
    return dict(lay_press_pa=view(rng, *lead, L) * 1e4, lay_temp=view(rng, *lead, L, dtype=np.float64) * 100,
                amount=view(rng, *lead, S, L), taucont=view(rng, *lead, W, L), dtaucon=view(rng, *lead, W, npar, L))


def layers_exp(kw, n, npar=NPAR):
    """-> lp (n, L), lt (n, L), am (n, S, L), tc (n, W, L), dtc (n, W, NPAR, L) as the header lays them out"""
    return (f8(kw["lay_press_pa"]).reshape(n, L), f8(kw["lay_temp"]).reshape(n, L), f8(kw["amount"]).reshape(n, S, L),
            f8(kw["taucont"]).reshape(n, W, L), f8(kw["dtaucon"]).reshape(n, W, npar, L))


def paths(seed=2):
    rng = np.random.default_rng(seed)
    layinc = np.array([[2, 1], [1, 0], [0, 0]], dtype=np.int64)
    wide = np.zeros((LIMAX, 2 * P), dtype=np.int64); wide[:, ::2] = layinc
    return dict(NLAYIN=np.array([3, 2], dtype=np.int64), LAYINC=wide[:, ::2], SCALE=view(rng, LIMAX, P),
                EMTEMP=view(rng, LIMAX, P, dtype=np.float64) * 100)


def over_models(a, n):
    return f8(np.broadcast_to(f8(a)[None], (n,) + np.shape(a)))


IGAS = np.array([1, 0], dtype=np.int64)
XFAC = np.linspace(1.0, 2.0, 2 * W)[::2]
EMISS = np.linspace(0.5, 1.0, W).astype(np.float32)
NPRO = 2


def dspecin_of_map2pro(eng, dspec, npar, limax, p):
    """the dSPECIN slot of the ansfm_map2pro call that map2pro(dspec, ...) makes"""
    rec = eng._lib
    script, rec.script = rec.script, None
    try:
        eng.map2pro(dspec, W, NVMR, npar - NVMR - 2, NPRO, p, [limax] * p, np.zeros((limax, p), dtype=np.int32), np.ones((L, NPRO)),
                    np.ones((L, NPRO)), np.ones((L, NPRO)))
    finally:
        rec.script = script
    name, args = rec.calls[-1]
    assert name == "ansfm_map2pro" and args[1:5] == (W, npar, limax, p)
    return args[9]


def check_chain(eng, dspec, single_model, on_dev, shape):
    """_chain_dspec after a gradient entry, and what map2pro makes of it; shape = (NPAR, layer axis, path axis)"""
    if on_dev:
        assert dspec is None and eng._chain_dspec == ("device", W) + shape
        assert dspecin_of_map2pro(eng, None, *shape) is None
        return
    if not single_model:
        assert eng._chain_dspec is None and dspec.flags.writeable
        with pytest.raises(ValueError, match="no device-resident cirsradg result"):
            eng.map2pro(None, W, NVMR, shape[0] - NVMR - 2, NPRO, shape[2], None, None, None, None, None)
        return
    one = dspec if dspec.ndim == 4 else dspec[0]
    assert not one.flags.writeable and eng._chain_dspec == _fingerprint(one)
    assert dspecin_of_map2pro(eng, one, *shape) is None                    # the very array that was returned: chained
    cp = one.copy()
    ptr = dspecin_of_map2pro(eng, cp, *shape)
    assert ptr is not None and ptr.value == cp.ctypes.data
    with pytest.raises(ValueError, match="no device-resident cirsradg result"):
        eng.map2pro(None, W, NVMR, shape[0] - NVMR - 2, NPRO, shape[2], None, None, None, None, None)


MODELS = [(1, False), (1, True), (3, True)]


# ---- the optional-axis entries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,axis", MODELS)
def test_thermal(eng, n, axis):
    kw, pa = layers(n, axis), paths()
    lp, lt, am, tc, _ = layers_exp(kw, n)
    sol, emi = np.array([10.0, 20.0], dtype=np.float32), [30, 40]
    eng._lib.expect("ansfm_cirsrad_ck_thermal", 1, n, L, lp, lt, am, tc, P, LIMAX, i4(pa["NLAYIN"]), i4(pa["LAYINC"]),
                    over_models(pa["SCALE"], n), over_models(pa["EMTEMP"], n), np.full(n, 150.0), f8(EMISS), f8(XFAC), None,
                    f8(sol), f8(emi), f8(XFAC), Out(n, W, P))
    out = eng.cirsrad_ck_thermal(1, kw["lay_press_pa"], kw["lay_temp"], kw["amount"], kw["taucont"], pa["NLAYIN"], pa["LAYINC"],
                                 pa["SCALE"], pa["EMTEMP"], 150.0, EMISSIVITY=EMISS, SOLFLUX=XFAC, SOL_ANG=sol, EMISS_ANG=emi, xfac=XFAC)
    assert np.array_equal(out, Out(n, W, P).ramp if axis else Out(W, P).ramp)


def test_thermal_one_path_no_continuum_per_model_scale(eng):
    """1-D LAYINC is one path; taucont and the optional arrays may be None; SCALE / EMTEMP / TSURF may carry the models"""
    n = 3
    kw = layers(n)
    lp, lt, am, _, _ = layers_exp(kw, n)
    rng = np.random.default_rng(5)
    sc, et, ts = view(rng, n, LIMAX, 1), view(rng, n, LIMAX, 1), view(rng, n)
    eng._lib.expect("ansfm_cirsrad_ck_thermal", 0, n, L, lp, lt, am, None, 1, LIMAX, i4([3]), i4([[2], [1], [0]]), f8(sc), f8(et),
                    f8(ts), None, None, None, None, None, None, Out(n, W, 1))
    out = eng.cirsrad_ck_thermal(0, kw["lay_press_pa"], kw["lay_temp"], kw["amount"], None, 3, np.array([2, 1, 0]), sc, et, ts)
    assert np.array_equal(out, Out(n, W, 1).ramp)


@pytest.mark.parametrize("n,axis", MODELS)
def test_transmission(eng, n, axis):
    kw, pa = layers(n, axis), paths()
    lp, lt, am, tc, _ = layers_exp(kw, n)
    eng._lib.expect("ansfm_cirsrad_ck_transmission", n, L, lp, lt, am, tc, P, LIMAX, i4(pa["NLAYIN"]), i4(pa["LAYINC"]),
                    over_models(pa["SCALE"], n), f8(XFAC), Out(n, W, P))
    out = eng.cirsrad_ck_transmission(kw["lay_press_pa"], kw["lay_temp"], kw["amount"], kw["taucont"], pa["NLAYIN"], pa["LAYINC"],
                                      pa["SCALE"], xfac=XFAC)
    assert np.array_equal(out, Out(n, W, P).ramp if axis else Out(W, P).ramp)


@pytest.mark.parametrize("n,axis", MODELS)
def test_transmission_gradients(eng, n, axis):
    kw, pa = layers(n, axis), paths()
    o = (Out(n, W, P), Out(n, W, NPAR, LIMAX, P, base=1000.0))
    eng._lib.expect("ansfm_cirsradg_ck_transmission", n, L, *layers_exp(kw, n), NVMR, NPAR, i4(IGAS), P, LIMAX, i4(pa["NLAYIN"]),
                    i4(pa["LAYINC"]), over_models(pa["SCALE"], n), None, *o)
    spec, dspec = eng.cirsradg_ck_transmission(kw["lay_press_pa"], kw["lay_temp"], kw["amount"], kw["taucont"], kw["dtaucon"], NVMR,
                                               NPAR, IGAS, pa["NLAYIN"], pa["LAYINC"], pa["SCALE"])
    for got, e in zip((spec, dspec), o):
        assert np.array_equal(got, e.ramp if axis else e.ramp[0])
    check_chain(eng, dspec, n == 1, False, (NPAR, LIMAX, P))


@pytest.mark.parametrize("on_dev", [False, True])
@pytest.mark.parametrize("n,axis", MODELS)
def test_thermal_gradients(eng, n, axis, on_dev):
    kw, pa = layers(n, axis), paths()
    dev = on_dev and n == 1                  # more than one model: the gradients come back whatever was asked
    o = (Out(n, W, P), Out(n, W, NPAR, LIMAX, P, base=1000.0, null=dev), Out(n, W, P, base=5000.0))
    eng._lib.expect("ansfm_cirsradg_ck_thermal", 0, n, L, *layers_exp(kw, n), NVMR, NPAR, i4(IGAS), P, LIMAX, i4(pa["NLAYIN"]),
                    i4(pa["LAYINC"]), over_models(pa["SCALE"], n), over_models(pa["EMTEMP"], n), np.full(n, 150.0), f8(EMISS), f8(XFAC), *o)
    res = eng.cirsradg_ck_thermal(0, kw["lay_press_pa"], kw["lay_temp"], kw["amount"], kw["taucont"], kw["dtaucon"], NVMR, NPAR, IGAS,
                                  pa["NLAYIN"], pa["LAYINC"], pa["SCALE"], pa["EMTEMP"], 150.0, EMISS, XFAC, gradients_on_device=on_dev)
    for got, e in zip(res, o):
        assert (got is None) if e.null else np.array_equal(got, e.ramp if axis else e.ramp[0])
    check_chain(eng, res[1], n == 1, dev, (NPAR, LIMAX, P))


def cont_inputs(n, axis=True, seed=3, nd=ND):
    rng = np.random.default_rng(seed)
    lead = (n,) if axis else ()
    return dict(q=view(rng, *lead, L, NVMR), FRAC=view(rng, *lead, L), TOTAM=view(rng, *lead, L), DELH=view(rng, *lead, L),
                CONT=view(rng, *lead, L, nd), f4=view(rng, *lead, L, 4))


def cont_exp(c, n, mode, nd=ND):
    """use_cia, lay_q, lay_frac, lay_totam, lay_delh, use_dust, lay_cont, ray_mode, f4 of include/ansfm.h"""
    return (1, f8(c["q"]).reshape(n, L, NVMR), f8(c["FRAC"]).reshape(n, L), f8(c["TOTAM"]).reshape(n, L), f8(c["DELH"]).reshape(n, L),
            1, f8(c["CONT"]).reshape(n, L, nd), mode, f8(c["f4"]).reshape(n, L, 4) if mode == 4 else None)


@pytest.mark.parametrize("on_dev", [False, True])
@pytest.mark.parametrize("n,axis", MODELS)
def test_thermal_cont_gradients(eng, n, axis, on_dev):
    npar = NVMR + 2 + ND
    kw, pa, c = layers(n, axis), paths(), cont_inputs(n, axis)
    lp, lt, am, _, _ = layers_exp(kw, n)
    dev = on_dev and n == 1
    o = (Out(n, W, P), Out(n, W, npar, LIMAX, P, base=1000.0, null=dev), Out(n, W, P, base=5000.0))
    eng._lib.expect("ansfm_cirsradg_ck_thermal_cont", 0, n, L, lp, lt, am, *cont_exp(c, n, 4), NVMR, npar, i4(IGAS), P, LIMAX,
                    i4(pa["NLAYIN"]), i4(pa["LAYINC"]), over_models(pa["SCALE"], n), over_models(pa["EMTEMP"], n), np.full(n, -1.0),
                    None, None, *o)
    res = eng.cirsradg_ck_thermal_cont(0, kw["lay_press_pa"], kw["lay_temp"], kw["amount"], c["q"], c["FRAC"], c["TOTAM"], c["DELH"],
                                       c["CONT"], 4, c["f4"], NVMR, npar, IGAS, pa["NLAYIN"], pa["LAYINC"], pa["SCALE"], pa["EMTEMP"],
                                       -1.0, gradients_on_device=on_dev)
    for got, e in zip(res, o):
        assert (got is None) if e.null else np.array_equal(got, e.ramp if axis else e.ramp[0])
    check_chain(eng, res[1], n == 1, dev, (npar, LIMAX, P))


def test_thermal_cont_terms_off_and_variant_v(eng):
    """q = None: no CIA; CONT = None: no aerosols; variant 'v' is ray_mode 12 whatever IRAY says, and takes no f4"""
    n = 1
    kw, pa, c = layers(n), paths(), cont_inputs(n)
    lp, lt, am, _, _ = layers_exp(kw, n)
    eng._lib.expect("ansfm_cirsradg_ck_thermal_cont", 0, n, L, lp, lt, am, 0, None, None, f8(c["TOTAM"]), None, 0, None, 12, None,
                    NVMR, NPAR, i4(IGAS), P, LIMAX, i4(pa["NLAYIN"]), i4(pa["LAYINC"]), over_models(pa["SCALE"], n),
                    over_models(pa["EMTEMP"], n), np.full(n, -1.0), None, None, Out(n, W, P), Out(n, W, NPAR, LIMAX, P), Out(n, W, P))
    eng.cirsradg_ck_thermal_cont(0, kw["lay_press_pa"], kw["lay_temp"], kw["amount"], None, None, c["TOTAM"], None, None, 1, c["f4"],
                                 NVMR, NPAR, IGAS, pa["NLAYIN"], pa["LAYINC"], pa["SCALE"], pa["EMTEMP"], -1.0, variant="v")


# ---- single scattering -------------------------------------------------------------------------------------------------
def ss_tail(seed=4):
    rng = np.random.default_rng(seed)
    return dict(EMISSIVITY=EMISS, BRDF=view(rng, W, P), SOLFLUX=XFAC, SOL_ANG=np.array([10, 20]), EMISS_ANG=[30.0, 40.0], xfac=XFAC)


def ss_tail_exp(t):
    return f8(t["EMISSIVITY"]), f8(t["BRDF"]), f8(t["SOLFLUX"]), f8(t["SOL_ANG"]), f8(t["EMISS_ANG"]), f8(t["xfac"])


def test_singlescatt(eng):
    kw, pa, t = layers(1, False), paths(), ss_tail()
    rng = np.random.default_rng(6)
    tausca, phase = view(rng, W, L), view(rng, P, W, L)
    lp, lt, am, tc, _ = layers_exp(kw, 1)
    eng._lib.expect("ansfm_cirsrad_ck_singlescatt", 0, L, lp[0], lt[0], am[0], tc[0], f8(tausca), f8(phase), P, LIMAX,
                    i4(pa["NLAYIN"]), i4(pa["LAYINC"]), f8(pa["SCALE"]), f8(pa["EMTEMP"]), 150.0, *ss_tail_exp(t), Out(W, P))
    out = eng.cirsrad_ck_singlescatt(0, kw["lay_press_pa"], kw["lay_temp"], kw["amount"], kw["taucont"], tausca, phase, pa["NLAYIN"],
                                     pa["LAYINC"], pa["SCALE"], pa["EMTEMP"], np.float32(150.0), **t)
    assert np.array_equal(out, Out(W, P).ramp)


def ss_batch_paths(n, seed=7):
    rng = np.random.default_rng(seed)
    pa = paths()
    return dict(pa, SCALE=view(rng, n, LIMAX, P), EMTEMP=view(rng, n, LIMAX, P), TSURF=view(rng, n))


@pytest.mark.parametrize("n", [1, 3])
def test_singlescatt_batch(eng, n):
    kw, pa, t = layers(n), ss_batch_paths(n), ss_tail()
    rng = np.random.default_rng(6)
    tausca, phase = view(rng, n, W, L), view(rng, n, P, W, L)
    lp, lt, am, tc, _ = layers_exp(kw, n)
    eng._lib.expect("ansfm_cirsrad_ck_singlescatt_batch", 0, n, L, lp, lt, am, tc, f8(tausca), f8(phase), P, LIMAX, i4(pa["NLAYIN"]),
                    i4(pa["LAYINC"]), f8(pa["SCALE"]), f8(pa["EMTEMP"]), f8(pa["TSURF"]), *ss_tail_exp(t), Out(n, W, P))
    out = eng.cirsrad_ck_singlescatt_batch(0, kw["lay_press_pa"], kw["lay_temp"], kw["amount"], kw["taucont"], tausca, phase,
                                           pa["NLAYIN"], pa["LAYINC"], pa["SCALE"], pa["EMTEMP"], pa["TSURF"], **t)
    assert np.array_equal(out, Out(n, W, P).ramp)


def ss_cont_call(eng, src, n, **over):
    kw, pa, t, c = layers(n), ss_batch_paths(n), ss_tail(), cont_inputs(n)
    rng = np.random.default_rng(8)
    a = dict(ISPACE=0, lay_press_pa=kw["lay_press_pa"], lay_temp=kw["lay_temp"], amount=kw["amount"], **c, IRAY=4, **pa, **t)
    a["alpha_deg" if src else "phase_fn"] = view(rng, P) if src else view(rng, W, P, ND + 1)
    a.update(over)
    fn = eng.cirsrad_ck_singlescatt_batch_src if src else eng.cirsrad_ck_singlescatt_batch_cont
    return a, kw, c, lambda: fn(**a)


@pytest.mark.parametrize("src", [False, True])
@pytest.mark.parametrize("n", [1, 3])
def test_singlescatt_batch_cont_src(eng, n, src):
    a, kw, c, call = ss_cont_call(eng, src, n)
    lp, lt, am, _, _ = layers_exp(kw, n)
    eng._lib.expect("ansfm_cirsrad_ck_singlescatt_batch_" + ("src" if src else "cont"), 0, n, L, lp, lt, am, *cont_exp(c, n, 4), ND,
                    f8(a["alpha_deg" if src else "phase_fn"]), P, LIMAX, i4(a["NLAYIN"]), i4(a["LAYINC"]), f8(a["SCALE"]),
                    f8(a["EMTEMP"]), f8(a["TSURF"]), *ss_tail_exp(a), Out(n, W, P))
    assert np.array_equal(call(), Out(n, W, P).ramp)


# ---- the fused one-model gradient routes ----------------------------------------------------------------------------------
MIX = np.array([[0.5, 0.0], [0.25, 0.75]])
MIX_ROWS = (i4([0, 1, 3]), i4([0, 0, 1]), f8([0.5, 0.25, 0.75]))         # compressed rows of MIX: ptr, path, val


def fused_call(eng, route, on_dev=False, dtau_every_gas=None, **over):
    """-> (the public call, the C name, its expected arguments, its outputs, the chain's shape)"""
    kw, pa = layers(1, False), paths()
    lp, lt, am, tc, dtc = (a[0] for a in layers_exp(kw, 1))
    head = dict(lay_press_pa=kw["lay_press_pa"], lay_temp=kw["lay_temp"], amount=kw["amount"], taucont=kw["taucont"],
                dtaucon=kw["dtaucon"], NVMR=NVMR, NPAR=NPAR, igas_map=IGAS, gradients_on_device=on_dev, dtau_every_gas=dtau_every_gas)
    ehead = (L, lp, lt, am, tc, dtc, NVMR, NPAR, i4(IGAS))
    epath = (P, LIMAX, i4(pa["NLAYIN"]), i4(pa["LAYINC"]), f8(pa["SCALE"]))
    grad = lambda q: Out(W, NPAR, L, q, base=9000.0, null=on_dev) if q else Out(W, NPAR, L, base=9000.0, null=on_dev)
    if route == "transit":
        cw = np.array([0.25, 0.75], dtype=np.float32)
        a = dict(head, NLAYIN=pa["NLAYIN"], LAYINC=pa["LAYINC"], SCALE=pa["SCALE"], path_weight=cw)
        outs = (Out(W), Out(W, P, base=100.0), grad(0))
        exp, qq = (*ehead, *epath, f8(cw), *outs), 1
    elif route == "occultation":
        a = dict(head, NLAYIN=pa["NLAYIN"], LAYINC=pa["LAYINC"], SCALE=pa["SCALE"], mix=MIX, xfac=XFAC)
        outs = (Out(W, Q), Out(W, P, base=100.0), grad(Q))
        exp, qq = (*ehead, *epath, Q, *MIX_ROWS, f8(XFAC), *outs), Q
    elif route == "limb":
        a = dict(head, ISPACE=1, NLAYIN=pa["NLAYIN"], LAYINC=pa["LAYINC"], SCALE=pa["SCALE"], EMTEMP=pa["EMTEMP"], mix=MIX_ROWS)
        outs = (Out(W, Q), Out(W, P, base=100.0), grad(Q))
        exp, qq = (1, *ehead, *epath, f8(pa["EMTEMP"]), Q, *MIX_ROWS, None, *outs), Q
    else:
        seq = np.array([2, 1, 0], dtype=np.int64)
        a = dict(head, ISPACE=0, LAYINC=seq, SCALE=pa["SCALE"], EMTEMP=pa["EMTEMP"][:, 0], TSURF=150, EMISSIVITY=EMISS, mix=MIX, xfac=XFAC)
        outs = (Out(W, Q), Out(W, P, base=100.0), Out(W, Q, base=200.0), grad(Q))
        exp = (0, *ehead, LIMAX, i4(seq), f8(pa["EMTEMP"][:, 0]), P, f8(pa["SCALE"]), 150.0, f8(EMISS), Q, *MIX_ROWS, f8(XFAC), *outs)
        qq = Q
    a.update(over)
    fn = getattr(eng, "cirsradg_ck_" + route)
    return (lambda: fn(**a)), "ansfm_cirsradg_ck_" + route, exp, outs, (NPAR, L, qq)


ROUTES = ["transit", "occultation", "limb", "disc"]


@pytest.mark.parametrize("on_dev", [False, True])
@pytest.mark.parametrize("route", ROUTES)
def test_fused_routes(eng, route, on_dev):
    call, name, exp, outs, chain = fused_call(eng, route, on_dev)
    eng._chain_dspec = ("device", 1, 1, 1, 1)             # what an earlier call left
    eng._lib.expect(name, *exp)
    res = call()
    assert len(res) == len(outs)
    for got, e in zip(res, outs):
        assert (got is None) if e.null else np.array_equal(got, e.ramp)
    if on_dev:
        check_chain(eng, res[-1], True, True, chain)
    else:                                                     # only gradients_on_device arms the chain
        assert eng._chain_dspec is None and res[-1].flags.writeable


@pytest.mark.parametrize("rc", [0, 1])
@pytest.mark.parametrize("route", ROUTES + ["thermal"])
def test_shared_gas_gradient_is_armed_and_disarmed(eng, route, rc):
    dg = view(np.random.default_rng(9), W, L)
    if route == "thermal":
        kw, pa = layers(1, False), paths()
        name = "ansfm_cirsradg_ck_thermal"
        call = lambda: eng.cirsradg_ck_thermal(0, kw["lay_press_pa"], kw["lay_temp"], kw["amount"], kw["taucont"], kw["dtaucon"], NVMR,
                                               NPAR, IGAS, pa["NLAYIN"], pa["LAYINC"], pa["SCALE"], pa["EMTEMP"], 150.0,
                                               dtau_every_gas=dg)
    else:
        call, name, _, _, _ = fused_call(eng, route, dtau_every_gas=dg)
    rec = eng._lib
    rec.script, rec.rc = None, {name: rc}
    if rc:
        with pytest.raises(ValueError, match="ANSFM_ERR_INVALID: recorded"):
            call()
    else:
        call()
    assert [c[0] for c in rec.calls] == ["ansfm_set_shared_gas_gradient", name, "ansfm_set_shared_gas_gradient"]
    arm, disarm = rec.calls[0][1], rec.calls[2][1]
    assert arm[1] == L and C.string_at(arm[2].value, 8 * W * L) == f8(dg).tobytes()
    assert disarm[1:] == (0, None)


# ---- multiple scattering ----------------------------------------------------------------------------------------------------
def ms_inputs(n=None, npath=P, wfull=W, seed=10):
    """the arguments of cirsrad_ck_scatter (n = None) or cirsrad_ck_scatter_batch by name"""
    rng = np.random.default_rng(seed)
    lead = () if n is None else (n,)
    kw = layers(n or 1, n is not None)
    return dict(ISPACE=0, lay_press_pa=kw["lay_press_pa"], lay_temp=kw["lay_temp"], amount=kw["amount"], TAUCIA=view(rng, *lead, W, L),
                TAUDUST=view(rng, *lead, W, L), TAURAY=None, TAUSCAT=view(rng, *lead, W, L), phasarr=view(rng, ND, wfull, 2, NTH),
                lfrac=view(rng, *lead, W, ND, L), radg=view(rng, *lead, W, NMU), sol_angs=np.linspace(10, 20, npath).astype(np.float32),
                emiss_angs=np.linspace(30, 40, npath), aphis=np.arange(npath), solar=view(rng, W), lowbc=1,
                brdf_matrix=view(rng, W, NMU, NMU, NF + 1), mu1=view(rng, NMU), wt1=view(rng, NMU), nf=NF, nphi=101, iray=1, imie=0,
                xfac=XFAC)


def ms_geometry_exp(a, g=slice(None)):
    """ngeom, sol_angs .. imie of the scattering entries' shared tail"""
    sol = f8(a["sol_angs"])[g]
    return (sol.shape[0], f8(sol), f8(f8(a["emiss_angs"])[g]), f8(f8(a["aphis"])[g]), f8(a["solar"]), 1, f8(a["brdf_matrix"]), NMU,
            f8(a["mu1"]), f8(a["wt1"]), NF, 101, 1, 0, f8(a["xfac"]))


def ms_layers_exp(a, n):
    return f8(a["lay_press_pa"]).reshape(n, L), f8(a["lay_temp"]).reshape(n, L), f8(a["amount"]).reshape(n, S, L)


@pytest.mark.parametrize("spec_g", [False, True])
def test_scatter(eng, spec_g):
    a = ms_inputs()
    lp, lt, am = (x[0] for x in ms_layers_exp(a, 1))
    o = (Out(W, P), Out(W, G, P, base=500.0, null=not spec_g))
    eng._lib.expect("ansfm_cirsrad_ck_scatter", 0, L, lp, lt, am, f8(a["TAUCIA"]), f8(a["TAUDUST"]), None, f8(a["TAUSCAT"]), ND, NTH,
                    f8(a["phasarr"]), f8(a["lfrac"]), f8(a["radg"]), *ms_geometry_exp(a), *o)
    res = eng.cirsrad_ck_scatter(**a, return_spec_g=spec_g)
    if spec_g:
        assert np.array_equal(res[0], o[0].ramp) and np.array_equal(res[1], o[1].ramp)
    else:
        assert np.array_equal(res, o[0].ramp)


@pytest.mark.parametrize("spec_g", [False, True])
def test_scatter_17_geometries_are_two_calls(eng, spec_g):
    assert AnsfmEngine.MS_PATHS_PER_CALL == 16
    a = ms_inputs(npath=17)
    lp, lt, am = (x[0] for x in ms_layers_exp(a, 1))
    outs = []
    for k, g in enumerate((slice(0, 16), slice(16, 17))):
        p = g.stop - g.start
        outs.append((Out(W, p, base=1000.0 * k), Out(W, G, p, base=5000.0 + 1000.0 * k, null=not spec_g)))
        eng._lib.expect("ansfm_cirsrad_ck_scatter", 0, L, lp, lt, am, f8(a["TAUCIA"]), f8(a["TAUDUST"]), None, f8(a["TAUSCAT"]), ND, NTH,
                        f8(a["phasarr"]), f8(a["lfrac"]), f8(a["radg"]), *ms_geometry_exp(a, g), *outs[-1])
    res = eng.cirsrad_ck_scatter(**a, return_spec_g=spec_g)
    spec = res[0] if spec_g else res
    assert np.array_equal(spec, np.concatenate([o[0].ramp for o in outs], axis=1))
    if spec_g:
        assert np.array_equal(res[1], np.concatenate([o[1].ramp for o in outs], axis=2))


@pytest.mark.parametrize("wave_slice", [None, (2, 9)])
@pytest.mark.parametrize("n", [1, 3])
def test_scatter_batch(eng, n, wave_slice):
    a = ms_inputs(n, wfull=W if wave_slice is None else 9)
    exp = (0, n, L, *ms_layers_exp(a, n), f8(a["TAUCIA"]), f8(a["TAUDUST"]), None, f8(a["TAUSCAT"]), ND, NTH, f8(a["phasarr"]),
           f8(a["lfrac"]), f8(a["radg"]), *ms_geometry_exp(a), Out(n, W, P))
    if wave_slice is None:
        eng._lib.expect("ansfm_cirsrad_ck_scatter_batch", *exp)
    else:
        eng._lib.expect("ansfm_cirsrad_ck_scatter_batch_slice", *exp, 9, 2)
    assert np.array_equal(eng.cirsrad_ck_scatter_batch(**a, wave_slice=wave_slice), Out(n, W, P).ramp)


def rows_inputs(n, wfull=W, seed=11):
    rng = np.random.default_rng(seed)
    a = ms_inputs(n, wfull=wfull)
    for k in ("TAUCIA", "TAUDUST", "TAURAY", "TAUSCAT", "lfrac"):
        del a[k]
    R = 4
    return dict(a, cont_row=np.arange(n * L, dtype=np.int64).reshape(n, L) % R, TAUCIA_rows=view(rng, R, W), TAUDUST_rows=None,
                TAURAY_rows=view(rng, R, W), TAUSCAT_rows=view(rng, R, W), lfrac_rows=view(rng, R, ND, W)), R


@pytest.mark.parametrize("wave_slice", [None, (2, 9)])
@pytest.mark.parametrize("n", [1, 3])
def test_scatter_batch_rows(eng, n, wave_slice):
    w_begin, wfull = wave_slice or (0, W)
    a, R = rows_inputs(n, wfull)
    eng._lib.expect("ansfm_cirsrad_ck_scatter_batch_rows", 0, n, L, *ms_layers_exp(a, n), R, i4(a["cont_row"]), f8(a["TAUCIA_rows"]), None,
                    f8(a["TAURAY_rows"]), f8(a["TAUSCAT_rows"]), ND, NTH, f8(a["phasarr"]), f8(a["lfrac_rows"]), f8(a["radg"]),
                    *ms_geometry_exp(a), Out(n, W, P), wfull, w_begin)
    assert np.array_equal(eng.cirsrad_ck_scatter_batch_rows(**a, wave_slice=wave_slice), Out(n, W, P).ramp)


def ms_cont_call(eng, src, n, wave_slice=None, **over):
    a = ms_inputs(n, wfull=(wave_slice or (0, W))[1])
    for k in ("TAUCIA", "TAUDUST", "TAURAY", "TAUSCAT", "lfrac"):
        del a[k]
    c = cont_inputs(n)
    a.update(c, IRAY=4, wave_slice=wave_slice)
    if src:
        del a["phasarr"]
        a["theta_deg"] = np.array([0.0, 30.0, 90.0, 180.0], dtype=np.float32)
    a.update(over)
    fn = eng.cirsrad_ck_scatter_batch_src if src else eng.cirsrad_ck_scatter_batch_cont
    return a, c, lambda: fn(**a)


@pytest.mark.parametrize("src,wave_slice", [(False, None), (False, (2, 9)), (True, None)])
@pytest.mark.parametrize("n", [1, 3])
def test_scatter_batch_cont_src(eng, n, src, wave_slice):
    a, c, call = ms_cont_call(eng, src, n, wave_slice)
    w_begin, wfull = wave_slice or (0, W)
    theta = f8(a["theta_deg"]) if src else None
    phase = (theta, f8(np.cos(theta * np.pi / 180))) if src else (f8(a["phasarr"]),)
    eng._lib.expect("ansfm_cirsrad_ck_scatter_batch_" + ("src" if src else "cont"), 0, n, L, *ms_layers_exp(a, n), *cont_exp(c, n, 4),
                    ND, NTH, *phase, f8(a["radg"]), *ms_geometry_exp(a), Out(n, W, P), wfull, w_begin)
    assert np.array_equal(call(), Out(n, W, P).ramp)


@pytest.mark.parametrize("rc", [0, 1])
@pytest.mark.parametrize("rows", [False, True])
def test_phase_variants_are_armed_and_disarmed(eng, rows, rc):
    n, V = 3, 3
    a = rows_inputs(n)[0] if rows else ms_inputs(n)
    po, pv = np.array([0, 2, 1], dtype=np.int64), view(np.random.default_rng(12), V - 1, ND, W, 2, NTH)
    name = "ansfm_cirsrad_ck_scatter_batch" + ("_rows" if rows else "")
    call = lambda **k: getattr(eng, name[len("ansfm_"):])(**a, **k)
    rec = eng._lib
    rec.script, rec.rc = None, {name: rc}
    if rc:
        with pytest.raises(ValueError, match="ANSFM_ERR_INVALID"):
            call(phase_of=po, phasarr_variants=pv)
    else:
        call(phase_of=po, phasarr_variants=pv)
    assert [c[0] for c in rec.calls] == ["ansfm_set_phase_variants", name, "ansfm_set_phase_variants"]
    arm, disarm = rec.calls[0][1], rec.calls[2][1]
    assert arm[1:3] == (n, V) and arm[4:6] == (ND, NTH)
    assert C.string_at(arm[3].value, 4 * n) == i4(po).tobytes() and C.string_at(arm[6].value, f8(pv).nbytes) == f8(pv).tobytes()
    assert disarm[1:] == (0, 1, None, 0, 0, None)
    del rec.calls[:]
    rec.rc = {}
    call(phase_of=po, phasarr_variants=pv[:0])            # V - 1 = 0: the plain call, no setter
    assert [c[0] for c in rec.calls] == [name]


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _thermalg(eng, **over):
    kw, pa = layers(1, False), paths()
    a = dict(ISPACE=0, lay_press_pa=kw["lay_press_pa"], lay_temp=kw["lay_temp"], amount=kw["amount"], taucont=kw["taucont"],
             dtaucon=kw["dtaucon"], NVMR=NVMR, NPAR=NPAR, igas_map=IGAS, **pa, TSURF=150.0)
    a.update(over)
    return eng.cirsradg_ck_thermal(**a)


def _ss_batch(eng, **over):
    n = 3
    kw, pa, t = layers(n), ss_batch_paths(n), ss_tail()
    rng = np.random.default_rng(6)
    a = dict(ISPACE=0, lay_press_pa=kw["lay_press_pa"], lay_temp=kw["lay_temp"], amount=kw["amount"], taucont=kw["taucont"],
             tausca=view(rng, n, W, L), phase=view(rng, n, P, W, L), **pa, **t)
    a.update(over)
    return eng.cirsrad_ck_singlescatt_batch(**a)


_ss_cont = lambda eng, src=False, **over: ss_cont_call(eng, src, 3, **over)[3]()
_fused = lambda eng, route, **over: fused_call(eng, route, **over)[0]()
_ms = lambda eng, **over: eng.cirsrad_ck_scatter(**dict(ms_inputs(), **over))
_ms_batch = lambda eng, **over: eng.cirsrad_ck_scatter_batch(**dict(ms_inputs(3), **over))
_ms_rows = lambda eng, **over: eng.cirsrad_ck_scatter_batch_rows(**dict(rows_inputs(3)[0], **over))
_ms_cont = lambda eng, src=False, **over: ms_cont_call(eng, src, 3, **over)[2]()
_z = np.zeros

REFUSALS = {
    "ss_batch: one model's layers": ("lay_press_pa", lambda e: _ss_batch(e, lay_press_pa=_z(L))),
    "ss_batch: amount": ("amount", lambda e: _ss_batch(e, amount=_z((3, S + 1, L)))),
    "ss_batch: TSURF": ("TSURF", lambda e: _ss_batch(e, TSURF=_z(2))),
    "ss_cont: one model's layers": ("lay_press_pa", lambda e: _ss_cont(e, lay_press_pa=_z(L))),
    "ss_cont: amount": ("amount", lambda e: _ss_cont(e, amount=_z((3, S, L + 1)))),
    "ss_cont: lay_temp": ("lay_temp", lambda e: _ss_cont(e, lay_temp=_z(3 * L))),
    "ss_cont: NLAYIN": ("NLAYIN", lambda e: _ss_cont(e, NLAYIN=[3])),
    "ss_cont: TSURF": ("TSURF", lambda e: _ss_cont(e, TSURF=150.0)),
    "ss_cont: BRDF": ("BRDF", lambda e: _ss_cont(e, BRDF=_z((P, W)))),
    "ss_cont: SCALE transposed": ("SCALE", lambda e: _ss_cont(e, SCALE=_z((3, P, LIMAX)))),
    "ss_src: EMTEMP flat": ("EMTEMP", lambda e: _ss_cont(e, True, EMTEMP=_z(3 * LIMAX * P))),
    "ss_cont: no phase_fn": ("phase_fn", lambda e: _ss_cont(e, phase_fn=None)),
    "ss_src: no alpha_deg": ("alpha_deg", lambda e: _ss_cont(e, True, alpha_deg=None)),
    "cont: q": ("q must be", lambda e: _ss_cont(e, q=_z((3, L, NVMR + 1)))),
    "cont: CIA without FRAC": ("FRAC", lambda e: _ss_cont(e, FRAC=None)),
    "cont: Rayleigh without TOTAM": ("TOTAM", lambda e: _ss_cont(e, q=None, TOTAM=None)),
    "cont: IRAY 4 without f4": ("f4", lambda e: _ss_cont(e, f4=None)),
    "one model: a batch": ("one model", lambda e: _fused(e, "transit", lay_press_pa=_z((1, L)))),
    "one model: NLAYIN": ("NLAYIN", lambda e: _fused(e, "limb", NLAYIN=[3, 2, 1])),
    "mix: rows": ("mix must be", lambda e: _fused(e, "occultation", mix=(i4([0, 1, 2]), i4([0, 1, 0]), f8([1.0, 1.0, 1.0])))),
    "mix: dense": ("dense mix", lambda e: _fused(e, "limb", mix=_z((Q, P + 1)))),
    "dtau_every_gas": ("dtau_every_gas", lambda e: _fused(e, "transit", dtau_every_gas=_z((L, W + 1)))),
    "dtau_every_gas: a batch": ("dtau_every_gas", lambda e: _thermalg(e, dtau_every_gas=_z((W, L)), **layers(3))),
    "disc: a batch": ("one model", lambda e: _fused(e, "disc", lay_press_pa=_z((1, L)))),
    "disc: EMTEMP": ("EMTEMP", lambda e: _fused(e, "disc", EMTEMP=_z(LIMAX + 1))),
    "disc: no mix": ("mix is required", lambda e: _fused(e, "disc", mix=None)),
    "variants: one of the two": ("go together", lambda e: _ms_batch(e, phase_of=[0, 0, 0])),
    "variants: phase_of": ("phase_of must be", lambda e: _ms_batch(e, phase_of=[0.0, 1.0, 1.0], phasarr_variants=_z((1, ND, W, 2, NTH)))),
    "variants: phasarr_variants": ("phasarr_variants must be",
                                   lambda e: _ms_rows(e, phase_of=[0, 1, 1], phasarr_variants=_z((1, ND, W + 1, 2, NTH)))),
    "scatter: amount": ("amount", lambda e: _ms(e, amount=_z((S + 1, L)))),
    "scatter: angles on both sides": ("Emission angles",
                                      lambda e: _ms(e, **{k: np.linspace(80, 100, 17) for k in ("sol_angs", "emiss_angs", "aphis")})),
    "batch: amount": ("amount", lambda e: _ms_batch(e, amount=_z((3, S, L + 1)))),
    "batch: phasarr of the slice": ("phasarr must cover", lambda e: _ms_batch(e, wave_slice=(2, 9))),
    "rows: one model's layers": ("lay_press_pa", lambda e: _ms_rows(e, lay_press_pa=_z(L))),
    "rows: amount": ("amount", lambda e: _ms_rows(e, amount=_z((3, S, L + 1)))),
    "rows: lay_temp": ("lay_temp", lambda e: _ms_rows(e, lay_temp=_z(3 * L))),
    "rows: cont_row": ("cont_row", lambda e: _ms_rows(e, cont_row=_z((3, L)))),
    "rows: no lfrac_rows": ("lfrac_rows is needed", lambda e: _ms_rows(e, lfrac_rows=None)),
    "rows: TAURAY_rows": ("TAURAY_rows", lambda e: _ms_rows(e, TAURAY_rows=_z((4, W + 1)))),
    "rows: lfrac_rows": ("lfrac_rows must be", lambda e: _ms_rows(e, lfrac_rows=_z((4, ND + 1, W)))),
    "rows: radg": ("radg", lambda e: _ms_rows(e, radg=_z((3, W, NMU + 1)))),
    "rows: phasarr": ("phasarr must cover", lambda e: _ms_rows(e, wave_slice=(2, 9))),
    "ms_cont: one model's layers": ("lay_press_pa", lambda e: _ms_cont(e, lay_press_pa=_z(L))),
    "ms_cont: amount": ("amount", lambda e: _ms_cont(e, amount=_z((3, S, L + 1)))),
    "ms_cont: lay_temp": ("lay_temp", lambda e: _ms_cont(e, lay_temp=_z(3 * L))),
    "ms_cont: no CONT": ("CONT is needed", lambda e: _ms_cont(e, CONT=None)),
    "ms_cont: radg": ("radg", lambda e: _ms_cont(e, radg=_z((3, W, NMU + 1)))),
    "ms_cont: phasarr": ("phasarr must cover", lambda e: _ms_cont(e, wave_slice=(2, 9), phasarr=_z((ND, W, 2, NTH)))),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_wrong_shapes_are_value_errors_before_any_call(eng, case):
    fragment, call = REFUSALS[case]               # the fragment names what was refused: it pins the check that raised
    with pytest.raises(ValueError, match=fragment):
        call(eng)
    assert not [c for c in eng._lib.calls if c[0] != "ansfm_ktable_info"]


def test_return_codes_become_exceptions(eng):
    kw, pa = layers(1), paths()
    call = lambda: eng.cirsrad_ck_transmission(kw["lay_press_pa"], kw["lay_temp"], kw["amount"], None, pa["NLAYIN"], pa["LAYINC"],
                                               pa["SCALE"])
    eng._lib.script = None
    for rc, exc in ((1, ValueError), (4, ValueError), (5, NotImplementedError), (2, _lib.AnsfmError)):
        eng._lib.rc = {"ansfm_cirsrad_ck_transmission": rc}
        with pytest.raises(exc, match="cirsrad_ck_transmission: %s: recorded" % _lib.ERR_NAMES[rc]):
            call()


# ---- what the marshalling helpers changed on purpose -------------------------------------------------------------------------
SHORT_NLAYIN = {
    "cirsrad_ck_thermal": lambda e: e.cirsrad_ck_thermal(0, *[layers(1)[k] for k in ("lay_press_pa", "lay_temp", "amount", "taucont")],
                                                         [3], paths()["LAYINC"], paths()["SCALE"], paths()["EMTEMP"], 150.0),
    "cirsrad_ck_transmission": lambda e: e.cirsrad_ck_transmission(*[layers(1)[k] for k in ("lay_press_pa", "lay_temp", "amount", "taucont")],
                                                                   [3], paths()["LAYINC"], paths()["SCALE"]),
    "cirsradg_ck_transmission": lambda e: e.cirsradg_ck_transmission(*layers(1).values(), NVMR, NPAR, IGAS, [3], paths()["LAYINC"],
                                                                     paths()["SCALE"]),
    "cirsradg_ck_thermal": lambda e: _thermalg(e, NLAYIN=[3]),
    "cirsradg_ck_thermal_cont": lambda e: e.cirsradg_ck_thermal_cont(
        0, *[layers(1)[k] for k in ("lay_press_pa", "lay_temp", "amount")], None, None, cont_inputs(1)["TOTAM"], None, None, 1, None, NVMR,
        NPAR, IGAS, [3, 2, 1], paths()["LAYINC"], paths()["SCALE"], paths()["EMTEMP"], 150.0),
    "cirsrad_ck_singlescatt_batch": lambda e: _ss_batch(e, NLAYIN=[3]),
    "cirsrad_ck_singlescatt_batch_cont": lambda e: _ss_cont(e, NLAYIN=[3]),
    "cirsrad_ck_singlescatt_batch_src": lambda e: _ss_cont(e, True, NLAYIN=[3]),
    "cirsradg_ck_transit": lambda e: _fused(e, "transit", NLAYIN=[3]),
    "cirsradg_ck_occultation": lambda e: _fused(e, "occultation", NLAYIN=[3]),
    "cirsradg_ck_limb": lambda e: _fused(e, "limb", NLAYIN=[3]),
}


@pytest.mark.parametrize("entry", list(SHORT_NLAYIN) + ["cirsrad_ck_singlescatt"])
def test_difference_nlayin_is_checked_by_every_entry(eng, entry):
    """a short NLAYIN was a host read past its end inside the library in seven of the ten entries that take one"""
    if entry == "cirsrad_ck_singlescatt":
        kw, pa, t = layers(1, False), paths(), ss_tail()
        call = lambda e: e.cirsrad_ck_singlescatt(0, kw["lay_press_pa"], kw["lay_temp"], kw["amount"], None, _z((W, L)), _z((P, W, L)), [3],
                                                  pa["LAYINC"], pa["SCALE"], pa["EMTEMP"], 150.0, **t)
    else:
        call = SHORT_NLAYIN[entry]
    with pytest.raises(ValueError, match=entry + ": NLAYIN"):
        call(eng)
    assert not [c for c in eng._lib.calls if c[0] != "ansfm_ktable_info"]


def test_difference_batch_lay_temp_is_exact_and_path_scales_broadcast(eng):
    """every batch entry wants lay_temp (n_models, NLAY) as given (two of the five reshaped it), and takes SCALE / EMTEMP
    (LIMAX, NPATH) for all the models, which failed in reshape or in the shape check"""
    n = 3
    with pytest.raises(ValueError, match="lay_temp"):
        _ss_batch(eng, lay_temp=_z(n * L))
    with pytest.raises(ValueError, match="lay_temp"):
        _ms_batch(eng, lay_temp=_z(n * L))
    assert not eng._lib.calls
    pa = paths()
    kw, bp, t = layers(n), ss_batch_paths(n), ss_tail()
    rng = np.random.default_rng(6)
    tausca, phase = view(rng, n, W, L), view(rng, n, P, W, L)
    lp, lt, am, tc, _ = layers_exp(kw, n)
    eng._lib.expect("ansfm_cirsrad_ck_singlescatt_batch", 0, n, L, lp, lt, am, tc, f8(tausca), f8(phase), P, LIMAX, i4(pa["NLAYIN"]),
                    i4(pa["LAYINC"]), over_models(pa["SCALE"], n), over_models(pa["EMTEMP"], n), f8(bp["TSURF"]), *ss_tail_exp(t),
                    Out(n, W, P))
    _ss_batch(eng, SCALE=pa["SCALE"], EMTEMP=pa["EMTEMP"])
    a, kw, c, call = ss_cont_call(eng, False, n, SCALE=pa["SCALE"], EMTEMP=pa["EMTEMP"])
    eng._lib.expect("ansfm_cirsrad_ck_singlescatt_batch_cont", 0, n, L, lp, lt, am, *cont_exp(c, n, 4), ND, f8(a["phase_fn"]), P, LIMAX,
                    i4(pa["NLAYIN"]), i4(pa["LAYINC"]), over_models(pa["SCALE"], n), over_models(pa["EMTEMP"], n), f8(a["TSURF"]),
                    *ss_tail_exp(a), Out(n, W, P))
    call()


@pytest.mark.parametrize("entry", ["cirsradg_ck_thermal", "cirsradg_ck_transmission"])
def test_difference_a_failed_gradient_call_leaves_no_chain(eng, entry):
    """the chain is cleared before the library call: after a failure map2pro(None, ...) has nothing to continue from"""
    eng._lib.script = None
    _thermalg(eng, gradients_on_device=True)
    assert eng._chain_dspec == ("device", W, NPAR, LIMAX, P)
    eng._lib.rc = {"ansfm_" + entry: 2}
    with pytest.raises(_lib.AnsfmError):
        if entry == "cirsradg_ck_thermal":
            _thermalg(eng)
        else:
            eng.cirsradg_ck_transmission(*layers(1).values(), NVMR, NPAR, IGAS, paths()["NLAYIN"], paths()["LAYINC"], paths()["SCALE"])
    with pytest.raises(ValueError, match="no device-resident cirsradg result"):
        eng.map2pro(None, W, NVMR, 0, NPRO, P, None, None, None, None, None)
