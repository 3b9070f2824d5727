"""ansfm_calc_phase / ansfm_calc_phase_ray / ansfm_upload_phase / ansfm_phase_from_source on the GPU (Scatter_0.calc_phase and
calc_phase_ray) against the reference's results in tests/golden/phase.npz.  The tabulated mode (IMIE 1) has neither cos nor
pow and is compared with np.array_equal; for the others the deviation relative to the column maximum over the angles stays
within 16 x `ulp`, the file's measure of what one ulp in every cos and pow is worth on the host, times the project's factor
for a few ulp per device transcendental (tests/test_brdf_gpu.py); never measured on the kernel.  Then: the resident source
gives the bits of the array-level entry, f_w / g1_w / g2_w those of np.interp, a repeated call the same bits, a case alone the
bits it has in a joint call, and the refusals by return code (nothing is provoked on the device)."""
import ctypes as C
import os

import numpy as np
import pytest

import phase_cases as pc

pytestmark = pytest.mark.gpu

CASES = ("hg-2x1", "hg-7pop", "mie-nodes", "mie-paths", "lp-1", "lp-2", "lp-36", "ray", "um")
INVALID, NOTABLE, UNSUPPORTED = 1, 3, 5


@pytest.fixture(scope="module")
def golden(golden_dir):
    return pc.load_golden(os.path.join(golden_dir, "phase.npz"))


@pytest.fixture(scope="module")
def engine():
    from archnemesis_dist_amd.engine import AnsfmEngine
    eng = AnsfmEngine(0)
    yield eng
    eng.close()


def run(engine, d, theta=None, wave=None, tab=None):
    if "imie" not in d:
        return engine.calc_phase_ray(d["theta"] if theta is None else theta)
    return engine.calc_phase(int(d["imie"]), d["swave"], d["ttab"], d["tab"] if tab is None else tab,
                             d["theta"] if theta is None else theta, d["wave"] if wave is None else wave)


def table_on(engine, wave):
    """a small k-table whose grid is `wave`: the resident source lives on it"""
    import singlescatt_cases as sc
    t = sc.synthetic_table("sorted", len(wave), 4, 3)
    t["WAVE"] = np.ascontiguousarray(wave, dtype=np.float64)
    sc.upload(engine, t)


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(engine, golden, name):
    d = golden[name]
    got = run(engine, d)
    ref, bound = d["ref"], 16 * float(d["ulp"])
    assert got.shape == ref.shape
    dev = pc.deviation(got, ref)
    print("%s: deviation / column maximum %.2e (bound %.2e), kernel %.3f ms" % (name, dev, bound, engine.phase_last()))
    if int(d.get("imie", -1)) in pc.EXACT_KINDS:
        assert np.array_equal(got, ref)
    else:
        assert dev <= bound
    assert np.array_equal(run(engine, d), got)              # a repeated call: the same bits


@pytest.mark.parametrize("name", ["lp-36", "hg-7pop", "mie-paths", "um"])      # W = 70, 67, 130, 33
def test_source_gives_the_bits_of_the_array_entry(engine, golden, name):
    d, other = golden[name], golden["mie-paths" if name != "mie-paths" else "lp-36"]
    inside = (d["wave"] >= d["swave"][0]) & (d["wave"] <= d["swave"][-1])
    wave = d["wave"][inside]
    table_on(engine, wave)
    want = run(engine, d, wave=wave)
    engine.upload_phase(int(d["imie"]), d["swave"], d["ttab"], d["tab"])
    first = engine.phase_from_source(d["theta"])
    assert np.array_equal(first, want)
    # another upload in between (its grid must cover the table's: scale the other case's onto it)
    sw = np.interp(other["swave"], other["swave"][[0, -1]], d["swave"][[0, -1]])
    engine.upload_phase(int(other["imie"]), sw, other["ttab"], other["tab"])
    assert engine.phase_from_source(other["theta"]).shape == (len(wave), len(other["theta"]), other["tab"].shape[2])
    engine.upload_phase(int(d["imie"]), d["swave"], d["ttab"], d["tab"])
    assert np.array_equal(engine.phase_from_source(d["theta"]), first)
    if int(d["imie"]) == 0:                                 # the slots of the scattering array: np.interp's bits
        th = np.array([0.0, 45.0, 90.0, 180.0])
        arr = engine.phasarr_from_source(th)
        hg = pc.hg_on_grid(d["swave"], d["tab"], wave)
        assert arr.shape == (d["tab"].shape[2], len(wave), 2, 4)
        assert np.array_equal(arr[:, :, 0, :3], np.transpose(hg, (1, 2, 0))) and not arr[:, :, 0, 3:].any()
        assert np.array_equal(arr[:, :, 1, :], np.broadcast_to(np.cos(th * np.pi / 180)[::-1], arr[:, :, 1, :].shape))
    else:
        th = d["ttab"] if int(d["imie"]) == 1 else pc.THETA41
        arr = engine.phasarr_from_source(th)
        assert np.array_equal(arr[:, :, 0, ::-1], np.transpose(engine.phase_from_source(th), (2, 0, 1)))
        assert np.array_equal(arr[:, :, 1, :], np.broadcast_to(np.cos(th * np.pi / 180)[::-1], arr[:, :, 1, :].shape))


def test_hg_on_the_grid_at_nodes_and_ends(engine, golden):
    """np.interp's rule: a node returns its tabulated value, beyond the ends the end values"""
    d = golden["hg-2x1"]
    wave = np.array([d["swave"][0], 900.0, 1000.3, d["swave"][1]])
    table_on(engine, wave)
    engine.upload_phase(0, d["swave"], None, d["tab"])
    arr = engine.phasarr_from_source(np.array([0.0, 90.0, 180.0]))
    assert np.array_equal(arr[:, :, 0, :], np.transpose(pc.hg_on_grid(d["swave"], d["tab"], wave), (1, 2, 0)))
    assert np.array_equal(arr[0, [0, 3], 0, :], d["tab"][:, [0, 1], 0].T)


def test_a_case_alone_gives_the_bits_of_the_joint_call(engine, golden):
    d = golden["hg-7pop"]
    full = run(engine, d)
    for pop in (0, 3, 6):
        assert np.array_equal(run(engine, d, tab=np.ascontiguousarray(d["tab"][:, :, pop:pop + 1]))[:, :, 0], full[:, :, pop])
    d = golden["mie-paths"]
    full = run(engine, d)
    for t in range(len(d["theta"])):
        assert np.array_equal(run(engine, d, theta=d["theta"][t:t + 1])[:, 0], full[:, t])
    assert np.array_equal(run(engine, d, wave=d["wave"][64:65])[0], full[64])
    d = golden["lp-36"]
    assert np.array_equal(run(engine, d, theta=d["theta"][7:8])[:, 0], run(engine, d)[:, 7])


def test_nine_populations_take_two_passes_of_the_legendre_sums(engine, golden):
    d = golden["lp-36"]
    tab = np.ascontiguousarray(np.concatenate([d["tab"]] * 5, axis=2)[:, :, :9] * np.linspace(1.0, 2.0, 9))
    got = run(engine, d, tab=tab)
    want = pc.calc_phase_np(2, d["swave"], d["ttab"], tab, d["theta"], d["wave"])
    assert got.shape == want.shape and pc.deviation(got, want) <= 16 * float(d["ulp"])
    assert np.array_equal(got[:, :, 8], run(engine, d, tab=np.ascontiguousarray(tab[:, :, 8:9]))[:, :, 0])


def _raw(engine, name, *args):
    fn = getattr(engine._lib, name)
    conv = lambda a: a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a
    return fn(engine._ctx, *[conv(a) for a in args])


def test_refusals(engine, golden):
    """every refusal by return code, through the C-ABI where Python would catch it first; the context answers afterwards"""
    h, m = golden["hg-2x1"], golden["mie-nodes"]
    out = np.empty((64, 64, 8))

    def calc(imie=1, NWS=None, SWAVE=m["swave"], NDUST=2, NTAB=5, TT=m["ttab"], tab=m["tab"], nth=2, th=np.array([10.0, 20.0]),
             W=2, wave=np.array([1010.0, 1340.0]), o=out):
        return _raw(engine, "ansfm_calc_phase", imie, len(SWAVE) if NWS is None else NWS, SWAVE, NDUST, NTAB, TT, tab, nth, th, W, wave, o)

    assert calc() == 0
    for kw in (dict(SWAVE=None, NWS=4), dict(tab=None), dict(TT=None), dict(th=None), dict(wave=None), dict(o=None)):      # null pointers
        assert calc(**kw) == INVALID, kw
    for kw in (dict(NWS=1), dict(nth=0), dict(NDUST=0), dict(NTAB=1), dict(imie=2, NTAB=0), dict(W=0)):
        assert calc(**kw) == INVALID, kw
    assert calc(SWAVE=np.array([1000.0, 1100.0, 1100.0, 1350.0])) == INVALID                 # not strictly ascending
    assert calc(SWAVE=np.ascontiguousarray(m["swave"][::-1])) == INVALID
    assert calc(TT=np.array([0.0, 30.0, 30.0, 120.0, 180.0])) == INVALID
    assert calc(TT=np.array([5.0, 30.0, 75.0, 120.0, 170.0]), th=np.array([4.0, 20.0])) == INVALID      # an angle outside THETA
    assert calc(TT=np.array([5.0, 30.0, 75.0, 120.0, 170.0]), th=np.array([20.0, 171.0])) == INVALID
    assert calc(th=np.array([20.0, np.nan])) == INVALID
    assert calc(wave=np.array([1010.0, 1351.0])) == INVALID and calc(wave=np.array([999.0, 1340.0])) == INVALID      # the range test
    assert calc(wave=np.array([1000.0 * (1 - 5e-7), 1350.0 * (1 + 5e-7)])) == 0                           # inside its tolerance
    assert calc(imie=3) == INVALID and calc(imie=-1) == INVALID
    assert b"imie" in engine._lib.ansfm_last_error(engine._ctx)
    assert _raw(engine, "ansfm_calc_phase_ray", 0, np.array([1.0]), out) == INVALID
    assert _raw(engine, "ansfm_calc_phase_ray", 1, None, out) == INVALID
    # the source
    table_on(engine, np.array([1010.0, 1100.0, 1340.0]))
    up = lambda imie=1, SWAVE=m["swave"], NDUST=2, NTAB=5, TT=m["ttab"], tab=m["tab"]: \
        _raw(engine, "ansfm_upload_phase", imie, len(SWAVE), SWAVE, NDUST, NTAB, TT, tab)
    assert _raw(engine, "ansfm_phase_from_source", 1, np.array([10.0]), out) == INVALID                   # none uploaded
    assert up(SWAVE=np.array([1020.0, 1100.0, 1300.0, 1350.0])) == INVALID                                # the range test on the grid
    assert up(NDUST=8, tab=np.zeros((4, 5, 8))) == UNSUPPORTED
    assert up(imie=5) == INVALID and up(tab=None) == INVALID
    assert _raw(engine, "ansfm_phase_from_source", 1, np.array([10.0]), out) == INVALID                   # a refused upload leaves none
    assert up() == 0
    assert _raw(engine, "ansfm_phase_from_source", 1, np.array([181.0]), out) == INVALID
    assert _raw(engine, "ansfm_phase_from_source", 0, np.array([10.0]), out) == INVALID
    assert _raw(engine, "ansfm_phase_from_source", 1, np.array([10.0]), None) == INVALID
    assert _raw(engine, "ansfm_phasarr_from_source", 2, np.array([10.0, 20.0]), np.array([1.0, 1.0]), out) == INVALID
    got = engine.phase_from_source(np.array([10.0, 20.0]))
    assert np.array_equal(got, engine.calc_phase(1, m["swave"], m["ttab"], m["tab"], np.array([10.0, 20.0]), np.array([1010.0, 1100.0, 1340.0])))
    # Python's own checks
    with pytest.raises(ValueError):
        engine.calc_phase(0, h["swave"], None, h["tab"][:2], h["theta"], h["wave"])
    with pytest.raises(NotImplementedError):
        engine.upload_phase(1, m["swave"], m["ttab"], np.zeros((4, 5, 8)))
    with pytest.raises(ValueError, match="cover"):
        engine.calc_phase(0, h["swave"], None, h["tab"], h["theta"], h["wave"] * 1.1)
    assert np.array_equal(run(engine, m), m["ref"])          # the context answers afterwards


def test_a_new_table_and_clear_remove_the_source(engine, golden):
    m = golden["mie-nodes"]
    wave = np.array([1010.0, 1100.0, 1340.0])
    table_on(engine, wave)
    engine.upload_phase(1, m["swave"], m["ttab"], m["tab"])
    engine.phase_from_source(np.array([10.0]))
    table_on(engine, wave)
    with pytest.raises(ValueError, match="no phase-function source"):
        engine.phase_from_source(np.array([10.0]))
    engine.upload_phase(1, m["swave"], m["ttab"], m["tab"])
    engine.clear_continuum_sources()
    with pytest.raises(ValueError, match="no phase-function source"):
        engine.phase_from_source(np.array([10.0]))
    eng2 = type(engine)(0)                      # no table at all
    try:
        assert _raw(eng2, "ansfm_upload_phase", 1, 4, m["swave"], 2, 5, m["ttab"], m["tab"]) == NOTABLE
    finally:
        eng2.close()
