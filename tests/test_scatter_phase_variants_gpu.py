"""Per-model phase functions inside the multiple-scattering batch (ansfm_set_phase_variants): every spectrum of a
batch whose models differ in an aerosol population's phase function has the bits of a separate `cirsrad_ck_scatter` call with that
model's phasarr, and a layer is taken from model 0's doubling results exactly where the rule in include/ansfm.h says so.

Base case: W = 70 (two 64-wavenumber tiles of the lane kernels), G = 3, L = 12 (a multiple of the prefix step, so a model that
shares every layer starts at lstart == L), S = 3, two aerosol populations and Rayleigh, TAURAY > 0 everywhere; population 0 is
present in layers 5-6 only, population 1 in layers 2-9.  All comparisons are np.array_equal."""
import numpy as np
import pytest

from test_gpu_parity import _scatter_inputs
from test_scatter_wavenumber_shard import _batch_args
from test_scatter_rows import _rows, _single

pytestmark = pytest.mark.gpu

W, G, L, S = 70, 3, 12, 3
KERNELS = [(5, 2), (16, 3), (8, 2)]                     # lane kernels, matrix-core chains, padded to 16 streams
GEOMETRY = [(False, 0), (False, 1), (True, 0), (True, 1)]
POP0_LAYERS, POP1_LAYERS = (5, 6), tuple(range(2, 10))


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


def _upload(e, z):
    e.upload_ktable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"], z["DELG"])


def _populations(z, rng, layers_of):
    """TAUSCAT / TAUDUST / lfrac of z rebuilt with population c present in layers_of[c] only (exact zeros elsewhere)"""
    ncont = len(layers_of)
    clscat = np.zeros((W, L, ncont))
    for c, layers in enumerate(layers_of):
        for l in layers:
            clscat[:, l, c] = 10.0 ** rng.uniform(-4, -1.5, W)
    z["TAUSCAT"] = clscat.sum(axis=2)
    z["TAUDUST"] = z["TAUSCAT"] * rng.uniform(1.02, 1.5, (W, L))
    pos = z["TAUSCAT"] > 0
    z["lfrac"] = np.ascontiguousarray(np.transpose(np.where(pos[:, :, None], clscat / np.where(pos, z["TAUSCAT"], 1.0)[:, :, None], 0.0),
                                                   (0, 2, 1)))
    return z


def _other_phase(phasarr, c, w_from, imie, rng):
    """phasarr with population c's phase function replaced at the wavenumbers >= w_from (another asymmetry; the angles stay)"""
    ph = phasarr.copy()
    n = ph.shape[1] - w_from
    if imie == 0:                                       # f, g1, g2 in the first three slots
        ph[c, w_from:, 0, 0] = rng.uniform(0.6, 0.95, n); ph[c, w_from:, 0, 1] = rng.uniform(0.3, 0.8, n)
        ph[c, w_from:, 0, 2] = rng.uniform(-0.5, -0.1, n)
    else:
        mu = ph[c, w_from:, 1, :]
        gg = rng.uniform(0.2, 0.7, (n, 1))
        ph[c, w_from:, 0, :] = (1 - gg * gg) / (1 + gg * gg - 2 * gg * mu) ** 1.5 / (4 * np.pi)
    assert not np.array_equal(ph[c, w_from:], phasarr[c, w_from:])
    return ph


def _case(NMU, NF, up, lowbc, layers_of=(POP0_LAYERS, POP1_LAYERS)):
    imie = 0 if NMU == 5 else 1                         # the double Henyey-Greenstein form on the lane kernels, tables on the others
    rng = np.random.default_rng(9100 + NMU + 7 * NF + 11 * lowbc + 13 * up)
    z = _populations(_scatter_inputs(rng, W, G, L, S, NMU, NF, 2, imie, 1, lowbc), rng, layers_of)
    assert (z["TAURAY"] > 0).all()
    return z, imie, rng


def _six_models(z, imie, rng):
    """-> (the batch's arrays, phase_of, the three variants): the table of the issue, model by model"""
    n = 6
    rep = lambda a: np.repeat(np.asarray(a)[None], n, 0).copy()
    b = dict(lay_press_pa=rep(z["lay_p"]), lay_temp=rep(z["lay_t"]), amount=rep(z["amount"]), TAUCIA=rep(z["TAUCIA"]),
             TAUDUST=rep(z["TAUDUST"]), TAURAY=rep(z["TAURAY"]), TAUSCAT=rep(z["TAUSCAT"]), lfrac=rep(z["lfrac"]), radg=rep(z["radg"]))
    b["lay_temp"][1, 4] *= 1.05                                             # 1: one layer's temperature
    for m in (2, 3):                                                        # 2, 3: population 0 changes in its layers 5-6
        sc0 = z["TAUSCAT"][:, 5:7] * z["lfrac"][:, 0, 5:7] * 1.3
        sc1 = z["TAUSCAT"][:, 5:7] * z["lfrac"][:, 1, 5:7]
        b["TAUSCAT"][m][:, 5:7] = sc0 + sc1
        b["TAUDUST"][m][:, 5:7] = z["TAUDUST"][:, 5:7] * 1.4
        b["lfrac"][m][:, 0, 5:7] = sc0 / (sc0 + sc1); b["lfrac"][m][:, 1, 5:7] = sc1 / (sc0 + sc1)
    b["amount"][3, 1, 2] *= 1.05                                            # 3: and a gas amount in layer 2
    variants = [z["phasarr"], _other_phase(z["phasarr"], 0, 0, imie, rng),  # 1: population 0 at every wavenumber
                _other_phase(z["phasarr"], 1, 30, imie, rng)]               # 2: population 1 from wavenumber 30 on
    return b, np.array([0, 0, 1, 1, 2, 1], dtype=np.int32), variants


def _predicted_hits(args, phase_of, variants):
    """(model, layer) pairs of models 1 .. n-1 that stay model 0's: every input of the layer has model 0's bits (the lower boundary
    is not a layer) and no population whose phase function differs from variant 0's has a non-zero fraction in it"""
    n = args["lay_press_pa"].shape[0]
    hits = 0
    for m in range(1, n):
        changed = [c for c in range(variants[0].shape[0]) if not np.array_equal(variants[phase_of[m]][c], variants[0][c])]
        for l in range(L):
            same = all(np.array_equal(args[k][m][..., l], args[k][0][..., l]) for k in
                       ("lay_press_pa", "lay_temp", "amount", "TAUCIA", "TAUDUST", "TAURAY", "TAUSCAT", "lfrac"))
            hits += bool(same and all((args["lfrac"][m][:, c, l] == 0).all() for c in changed))
    return hits, (n - 1) * L


_SHARED = {}


def _shared(eng, NMU, NF, up, lowbc):
    """One base case per parametrisation: the arguments, the variants and the separate calls, computed once and left unchanged"""
    key = (NMU, NF, up, lowbc)
    if key not in _SHARED:
        z, imie, rng = _case(NMU, NF, up, lowbc)
        b, phase_of, variants = _six_models(z, imie, rng)
        args = _batch_args(z, b, up, lowbc, NF, iray=1, imie=imie)
        _upload(eng, z)
        singles = np.stack([_single(eng, dict(args, phasarr=variants[phase_of[m]]), m) for m in range(6)])
        for a in (singles, phase_of, *variants):
            a.setflags(write=False)
        _SHARED[key] = dict(z=z, args=args, phase_of=phase_of, variants=variants, singles=singles,
                            kw=dict(phase_of=phase_of, phasarr_variants=np.stack(variants[1:])))
    _upload(eng, _SHARED[key]["z"])
    return _SHARED[key]


@pytest.mark.parametrize("NMU,NF", KERNELS)
@pytest.mark.parametrize("up,lowbc", GEOMETRY)
def test_variants_equal_separate_calls(eng, NMU, NF, up, lowbc):
    c = _shared(eng, NMU, NF, up, lowbc)
    got = eng.cirsrad_ck_scatter_batch(**c["args"], **c["kw"])
    hits = eng.last_scatter_cache()
    for m in range(6):
        assert np.array_equal(got[m], c["singles"][m]), m
    # the rule as include/ansfm.h states it, not narrowed: model 5 recomputes layers 5-6 and takes the other ten from the cache
    want = _predicted_hits(c["args"], c["phase_of"], c["variants"])
    assert want == (11 + 10 + 9 + 4 + 10, 60)
    assert hits == want
    # two (variant, population) pairs were integrated and walked beside variant 0's three components; Rayleigh and the
    # unchanged population of each variant were not
    pairs, nbytes = eng.last_scatter_variants()
    nn = (16 if NMU >= 7 else NMU) ** 2
    assert pairs == 2 and nbytes == 2 * 8 * (2 * W * (NF + 1) * 3 * nn + G * W * 3 * nn)
    # the variants are distinguishable at all: model 5 differs from model 0 in nothing but the phase function
    assert not np.array_equal(got[5], got[0])


@pytest.mark.parametrize("NMU,NF", KERNELS)
@pytest.mark.parametrize("up,lowbc", GEOMETRY)
def test_rows_entry_equals_dense_entry(eng, NMU, NF, up, lowbc):
    c = _shared(eng, NMU, NF, up, lowbc)
    dense = eng.cirsrad_ck_scatter_batch(**c["args"], **c["kw"])
    hd = eng.last_scatter_cache()
    rows = eng.cirsrad_ck_scatter_batch_rows(**_rows(c["args"]), **c["kw"])
    assert np.array_equal(rows, dense)
    assert np.array_equal(rows, c["singles"])
    assert eng.last_scatter_cache() == hd == _predicted_hits(c["args"], c["phase_of"], c["variants"])


@pytest.mark.parametrize("NMU,NF", KERNELS)
@pytest.mark.parametrize("up,lowbc", GEOMETRY)
def test_model_that_shares_every_layer(eng, NMU, NF, up, lowbc):
    """Population 0 is absent from every layer and model 2 changes nothing but its phase function: model 0's bits, every layer
    from the cache, the sweep starts at lstart == L."""
    z, imie, rng = _case(NMU, NF, up, lowbc, layers_of=((), POP1_LAYERS))
    rep = lambda a: np.repeat(np.asarray(a)[None], 3, 0).copy()
    b = dict(lay_press_pa=rep(z["lay_p"]), lay_temp=rep(z["lay_t"]), amount=rep(z["amount"]), TAUCIA=rep(z["TAUCIA"]),
             TAUDUST=rep(z["TAUDUST"]), TAURAY=rep(z["TAURAY"]), TAUSCAT=rep(z["TAUSCAT"]), lfrac=rep(z["lfrac"]), radg=rep(z["radg"]))
    b["lay_temp"][1, 4] *= 1.05
    args = _batch_args(z, b, up, lowbc, NF, iray=1, imie=imie)
    other = _other_phase(z["phasarr"], 0, 0, imie, rng)
    _upload(eng, z)
    kw = dict(phase_of=np.array([0, 0, 1], dtype=np.int32), phasarr_variants=other[None])
    for entry, a in ((eng.cirsrad_ck_scatter_batch, args), (eng.cirsrad_ck_scatter_batch_rows, _rows(args))):
        got = entry(**a, **kw)
        assert np.array_equal(got[2], got[0])
        assert eng.last_scatter_cache() == (11 + 12, 24)
        assert eng.last_scatter_variants()[0] == 1
    assert np.array_equal(got[2], _single(eng, dict(args, phasarr=other), 2))
    assert np.array_equal(got[1], _single(eng, args, 1))


@pytest.mark.parametrize("NMU,NF", KERNELS)
def test_no_variant_in_use_is_the_plain_call_and_the_setting_is_consumed(eng, NMU, NF):
    c = _shared(eng, NMU, NF, False, 1)
    plain = eng.cirsrad_ck_scatter_batch(**c["args"])
    hp = eng.last_scatter_cache()
    assert eng.last_scatter_variants() == (0, 0)
    zeros = eng.cirsrad_ck_scatter_batch(**c["args"], phase_of=np.zeros(6, dtype=np.int32), phasarr_variants=c["kw"]["phasarr_variants"])
    assert np.array_equal(zeros, plain) and eng.last_scatter_cache() == hp
    v1 = eng.cirsrad_ck_scatter_batch(**c["args"], phase_of=np.zeros(6, dtype=np.int32),
                                      phasarr_variants=np.empty((0,) + c["variants"][0].shape))
    assert np.array_equal(v1, plain) and eng.last_scatter_cache() == hp
    with_variants = eng.cirsrad_ck_scatter_batch(**c["args"], **c["kw"])
    assert not np.array_equal(with_variants, plain)
    after = eng.cirsrad_ck_scatter_batch(**c["args"])
    assert np.array_equal(after, plain) and eng.last_scatter_cache() == hp and eng.last_scatter_variants() == (0, 0)
    assert np.array_equal(eng.cirsrad_ck_scatter_batch_rows(**_rows(c["args"])), plain)


@pytest.mark.parametrize("NMU,NF", KERNELS)
@pytest.mark.parametrize("up,lowbc", GEOMETRY)
def test_model_by_model_route(eng, NMU, NF, up, lowbc):
    c = _shared(eng, NMU, NF, up, lowbc)
    eng.set_layer_dedup(False)
    try:
        dense = eng.cirsrad_ck_scatter_batch(**c["args"], **c["kw"])
        rows = eng.cirsrad_ck_scatter_batch_rows(**_rows(c["args"]), **c["kw"])
    finally:
        eng.set_layer_dedup(True)
    assert np.array_equal(dense, c["singles"])
    assert np.array_equal(rows, c["singles"])


def test_layer_cache_switched_off_by_the_environment(eng, monkeypatch):
    c = _shared(eng, 16, 3, False, 1)
    monkeypatch.setenv("ANSFM_MS_LAYER_CACHE", "0")
    assert np.array_equal(eng.cirsrad_ck_scatter_batch(**c["args"], **c["kw"]), c["singles"])


def _raw_pending(eng, c):
    """arms the six models' variants through the C entry alone"""
    from archnemesis_dist_amd.engine import _ptr
    po, pv = c["kw"]["phase_of"], np.ascontiguousarray(c["kw"]["phasarr_variants"])
    assert eng._lib.ansfm_set_phase_variants(eng._ctx, 6, 3, _ptr(po), pv.shape[1], pv.shape[4], _ptr(pv)) == 0


def test_refusals_leave_the_next_call_alone(eng):
    from archnemesis_dist_amd import _lib
    c = _shared(eng, 16, 3, False, 1)
    args, kw = c["args"], c["kw"]
    plain = eng.cirsrad_ck_scatter_batch(**args)

    def unaffected():
        assert np.array_equal(eng.cirsrad_ck_scatter_batch(**args), plain)
        assert eng.last_scatter_variants() == (0, 0)

    with pytest.raises(ValueError, match="INVALID.*outside"):
        eng.cirsrad_ck_scatter_batch(**args, phase_of=np.array([0, 0, 1, 3, 2, 1], dtype=np.int32), phasarr_variants=kw["phasarr_variants"])
    unaffected()
    with pytest.raises(ValueError, match="INVALID.*outside"):
        eng.cirsrad_ck_scatter_batch_rows(**_rows(args), phase_of=np.array([0, 0, -1, 1, 2, 1], dtype=np.int32),
                                          phasarr_variants=kw["phasarr_variants"])
    unaffected()
    with pytest.raises(ValueError, match=r"INVALID.*phase_of\[0\]"):
        eng.cirsrad_ck_scatter_batch(**args, phase_of=np.array([1, 0, 1, 1, 2, 1], dtype=np.int32), phasarr_variants=kw["phasarr_variants"])
    unaffected()
    with pytest.raises(ValueError, match="INVALID.*n_models"):
        eng.cirsrad_ck_scatter_batch(**args, phase_of=kw["phase_of"][:5], phasarr_variants=kw["phasarr_variants"])
    unaffected()
    # the `_cont` entry: the refusal comes before any of its arguments is read
    _raw_pending(eng, c)
    proto = _lib.PROTOTYPES["ansfm_cirsrad_ck_scatter_batch_cont"][1]
    import ctypes as C
    rc = eng._lib.ansfm_cirsrad_ck_scatter_batch_cont(eng._ctx, *(None if t is C.c_void_p else 0 for t in proto[1:]))
    with pytest.raises(NotImplementedError, match="UNSUPPORTED.*no model axis"):
        eng._check(rc, "cirsrad_ck_scatter_batch_cont")
    unaffected()
    # a slice: the table is the first W wavenumbers of a longer axis
    longer = np.concatenate([args["phasarr"], args["phasarr"][:, :10]], axis=1)
    with pytest.raises(NotImplementedError, match="UNSUPPORTED.*slice"):
        eng.cirsrad_ck_scatter_batch(**dict(args, phasarr=longer), wave_slice=(0, W + 10), **kw)
    unaffected()
    with pytest.raises(NotImplementedError, match="UNSUPPORTED.*slice"):
        eng.cirsrad_ck_scatter_batch_rows(**dict(_rows(args), phasarr=longer), wave_slice=(0, W + 10), **kw)
    unaffected()


def test_one_g_ordinate_is_refused(eng):
    """G = 1 (an LBL table): the windowed walk with carries has no variants"""
    from test_lbl_scatter import _lbl_inputs
    rng = np.random.default_rng(9400)
    Wl, NMU, NF = 70, 16, 2
    z = _lbl_inputs(rng, Wl, L, 2, NMU, NF, 1, 1, 1, 1)
    rep = lambda a: np.repeat(np.asarray(a)[None], 2, 0).copy()
    b = dict(lay_press_pa=rep(z["lay_p"]), lay_temp=rep(z["lay_t"]), amount=rep(z["amount"]), TAUCIA=rep(z["TAUCIA"]),
             TAUDUST=rep(z["TAUDUST"]), TAURAY=rep(z["TAURAY"]), TAUSCAT=rep(z["TAUSCAT"]), lfrac=rep(z["lfrac"]), radg=rep(z["radg"]))
    b["lay_temp"][1, 4] *= 1.05
    args = _batch_args(z, b, False, 1, NF)
    eng.upload_lbltable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"])
    plain = eng.cirsrad_ck_scatter_batch(**args)
    other = _other_phase(z["phasarr"], 0, 0, 1, rng)
    with pytest.raises(NotImplementedError, match="UNSUPPORTED.*one g-ordinate"):
        eng.cirsrad_ck_scatter_batch(**args, phase_of=np.array([0, 1], dtype=np.int32), phasarr_variants=other[None])
    assert np.array_equal(eng.cirsrad_ck_scatter_batch(**args), plain)
