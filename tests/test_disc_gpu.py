"""ansfm_cirsradg_ck_disc on the GPU (k_disc_planck, k_disc_sens, k_disc_grad): the thermal emission of the averaging points of an
unresolved planet -- paths through one layer sequence that differ in SCALE -- mixed to the geometries with their layer gradients
and the surface-temperature gradient, against the collapsed restatement (tests/disc_cases.py) on the CPU oracle's opacities,
against the un-collapsed route of the same engine (cirsradg_ck_thermal on the P paths, then the restatement's weighted sum,
sum C dTSURF included), against cirsradg_ck_limb where the sequence does not reach the ground, and against the reference's
nemesisdiscfmg in tests/golden/disc_c1.npz.

Tolerances are those test_limb_gpu.py holds this branch to: 1e-10 relative on a radiance, 1e-10 of the parameter slab's largest
element on a gradient.  MOD[w, q] = xfac sum_p C[q, p] SPEC_p inherits 1e-10 max|xfac| sum_p |C[q, p]| max SPEC, and
dTSMOD[w, q] = xfac sum_p C[q, p] dTSURF_p the same with the largest dTSURF_p in place of max SPEC."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import disc_cases as dc  # noqa: E402
import transit_cases as tc  # noqa: E402
from test_limb_gpu import _opacities, _upload, _wide_case as _limb_wide_case  # noqa: E402  (the oracle's opacities, cached by case)
from test_transit_gpu import _case as _transit_case  # noqa: E402  (the synthetic generator: G = 10, S = 3, or G = 1 on an LBL table)

pytestmark = pytest.mark.gpu

NVMR, NDUST = 4, 1
NPAR = NVMR + 2 + NDUST
IGAS_MAP = np.array([2, 0, 3], dtype=np.int32)
CAP = 160                       # layers of the fused call (include/ansfm.h)
CHUNK = 8                       # kDiscChunk of csrc/ansfm_disc_kernels.hip.h: paths that walk the sequence in lock-step


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


def _sequence(c, L, P, kind, rng):
    """ground: from the top layer down to layer 0 (the deepest: the lower boundary contributes); limb: down to layer 3 and up
    again (it does not).  EMTEMP: the layer's temperature moved by up to 3 K per entry; SCALE drawn per entry and path (ragged
    columns: no path is a multiple of another)."""
    if kind == "limb":
        LAYINC = np.concatenate([np.arange(L - 1, 2, -1), np.arange(3, L)]).astype(np.int32)
    else:
        LAYINC = np.arange(L - 1, -1, -1).astype(np.int32)
    N = LAYINC.size
    c["LAYINC"] = LAYINC
    c["EMTEMP"] = np.asarray(c["lt"])[LAYINC] + rng.uniform(-3.0, 3.0, N)
    c["SCALE"] = (1.0 / np.cos(np.radians(np.linspace(0.0, 70.0, P))))[None, :] * rng.uniform(0.9, 1.1, (N, P))
    assert dc.is_ground(c["lp"], LAYINC) == (kind != "limb")


def _mix(P, Q, rng):
    if Q == 1:
        w = rng.uniform(0.1, 1.0, (1, P))
        return w / w.sum()
    if Q == 9:
        # more geometries than the kMixWaves = 4 waves of a contraction block: rows of two or three weights on successive averaging
        # points, row 4 empty -- every geometry with a weight has an entry in every layer of the sequence, so each wave serves two
        assert P == 9
        C = np.zeros((Q, P))
        for q in (0, 1, 2, 3, 5, 6, 7, 8):
            n = 2 + q % 2
            C[q, (q + np.arange(n)) % P] = rng.uniform(0.1, 1.0, n)
        return C / np.where(C.sum(axis=1, keepdims=True) > 0, C.sum(axis=1, keepdims=True), 1.0)
    # neighbouring geometries share path 1, the last path is named by no geometry, the third row is empty, a negative weight
    assert Q == 3 and P == 4
    return np.array([[0.3, 0.7, 0.0, 0.0], [0.0, -0.55, 1.45, 0.0], [0.0, 0.0, 0.0, 0.0]])


@functools.lru_cache(maxsize=None)
def _case(W, L=12, lbl=False, P=3, Q=1, kind="ground"):
    t = _transit_case(W, L, lbl)
    rng = np.random.default_rng(11 + W + 1000 * L + 7 * P)
    c = {k: v for k, v in t.items() if k not in ("NLAYIN", "LAYINC", "SCALE", "weight")}
    _sequence(c, L, P, kind, rng)
    c["C"] = _mix(P, Q, rng)
    c["xfac"] = rng.uniform(0.5, 2.0, W) * 1.0e3
    c["emis"] = np.linspace(0.55, 0.95, W) if W > 1 else np.array([0.8])
    c["G"] = 1 if lbl else 10
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def _wide_case(G=20, S=16):
    """_wide_case of test_limb_gpu.py (L = 4, W = 64; G = 20, S = 16: 17 slots of 10 KiB beside 40 KiB of columns, more than one
    LDS stage holds; any other (G, S): a size case, its amounts scaled there), with a sequence to the ground and three paths"""
    w = _limb_wide_case(G, S)
    c = {k: v for k, v in w.items() if k not in ("NLAYIN", "LAYINC", "SCALE", "EMTEMP", "C")}
    rng = np.random.default_rng(93)
    c["lp"] = np.array(w["lp"])
    _sequence(c, c["L"], 3, "ground", rng)
    c["C"] = np.array([[0.2, 0.5, 0.3]])
    c["emis"] = np.linspace(0.55, 0.95, c["W"])
    return _freeze(c)


def _dims(c):
    return c.get("NVMR", NVMR), c.get("NPAR", NPAR), c.get("igas_map", IGAS_MAP)


def _fused(eng, c, dcont="dcont", xfac=True, ispace=0, tsurf=-1.0, **kw):
    nvmr, npar, ig = _dims(c)
    return eng.cirsradg_ck_disc(ispace, c["lp"], c["lt"], c["am"], c["cont"], None if dcont is None else c[dcont], nvmr, npar, ig,
                                c["LAYINC"], c["SCALE"], c["EMTEMP"], tsurf, EMISSIVITY=c["emis"] if tsurf > 0 else None, mix=c["C"],
                                xfac=c["xfac"] if xfac else None, **kw)


def _as_paths(c):
    """the sequence as cirsradg_ck_thermal / cirsradg_ck_limb take paths: NLAYIN (P,), LAYINC, SCALE, EMTEMP (N, P)"""
    N, P = c["SCALE"].shape
    return (np.full(P, N, dtype=np.int32), np.ascontiguousarray(np.tile(c["LAYINC"][:, None], (1, P))), c["SCALE"],
            np.ascontiguousarray(np.tile(c["EMTEMP"][:, None], (1, P))))


def _thermal(eng, c, dcont, xfac=True, ispace=0, tsurf=-1.0):
    nvmr, npar, ig = _dims(c)
    return eng.cirsradg_ck_thermal(ispace, c["lp"], c["lt"], c["am"], c["cont"], dcont, nvmr, npar, ig, *_as_paths(c), tsurf,
                                   EMISSIVITY=c["emis"] if tsurf > 0 else None, xfac=c["xfac"] if xfac else None)


def _uncollapsed_on_engine(eng, c, dcont, xfac=True, ispace=0, tsurf=-1.0):
    spec, dspec, dts = _thermal(eng, c, dcont, xfac, ispace, tsurf)
    MOD, dTSMOD, dMOD = dc.mod_from_points(spec, dspec, dts, c["C"], c["LAYINC"], c["L"])
    xf = c["xfac"][:, None] if xfac else 1.0
    return (MOD, spec / xf, dTSMOD, dMOD), np.abs(dts / xf).max()


def _compare(what, got, ref, C, xfmax, dts_max):
    (MOD, SPEC, dTSMOD, dMOD), (rM, rS, rT, rdM) = got, ref
    scale = np.max(np.abs(rdM), axis=(0, 2, 3), keepdims=True)
    err = np.max(np.abs(dMOD - rdM) / np.where(scale > 0, scale, 1.0), axis=(0, 2, 3))
    atol = 1e-10 * xfmax * np.abs(C).sum(axis=1) * rS.max()
    atol_ts = 1e-10 * xfmax * np.abs(C).sum(axis=1) * dts_max
    print("%s: SPEC rel %.3e, MOD / its bound %.3e, dTSMOD / its bound %.3e, dMOD by parameter %s" % (
        what, np.max(np.abs(SPEC - rS) / rS), np.max(np.abs(MOD - rM) / np.where(atol > 0, atol, 1.0)[None, :]),
        np.max(np.abs(dTSMOD - rT) / np.where(atol_ts > 0, atol_ts, 1.0)[None, :]), np.array2string(err, precision=2)))
    np.testing.assert_allclose(SPEC, rS, rtol=1e-10)
    assert np.all(np.abs(MOD - rM) <= atol[None, :])
    assert np.all(np.abs(dTSMOD - rT) <= atol_ts[None, :])
    assert err.max() < 1e-10
    assert np.all(dMOD[:, scale.reshape(-1) == 0] == 0.0)


def _check_case(eng, oracle, c, dcont="dcont", xfac=True, ispace=0, tsurf=-1.0, gases=None, temperature=True, every_gas=False):
    nvmr, npar, ig = _dims(c)
    _upload(eng, c)
    got = _fused(eng, c, dcont, xfac, ispace, tsurf, dtau_every_gas=c["dray"] if every_gas else None)
    Q, P = c["C"].shape
    W = c["W"]
    assert got[0].shape == (W, Q) and got[1].shape == (W, P) and got[2].shape == (W, Q) and got[3].shape == (W, npar, c["L"], Q)
    tautot, dk = _opacities(oracle, c)
    dtau = tc.dtautot(dk, ig, nvmr, npar, None if dcont is None else c[dcont], c["dray"] if every_gas else None,
                      gases=gases, temperature=temperature)
    xf = c["xfac"] if xfac else None
    emis = c["emis"] if tsurf > 0 else None
    seq = (tautot, np.asarray(c["delg"], dtype=np.float64), c["lp"], c["LAYINC"], c["SCALE"], c["EMTEMP"], tsurf, emis)
    ref = dc.collapsed(*seq, c["C"], ispace, c["WAVE"], nvmr, dtau, xf)
    dts_max = np.abs(dc.uncollapsed(*seq, ispace, c["WAVE"], nvmr)[2]).max()          # per path, before xfac
    assert np.abs(ref[3]).max() > 0 and ref[1].min() > 1e-300
    xfmax = float(np.abs(c["xfac"]).max()) if xfac else 1.0
    _compare("oracle, collapsed", got, ref, c["C"], xfmax, dts_max)
    dcn = None if dcont is None else np.array(c[dcont])
    if every_gas:                                        # the un-collapsed call takes the shared term inside dtaucon
        dcn = np.zeros((W, npar, c["L"])) if dcn is None else dcn
        dcn[:, :nvmr, :] += c["dray"][:, None, :]
    unc, unc_dts = _uncollapsed_on_engine(eng, c, dcn, xfac, ispace, tsurf)
    _compare("same engine, un-collapsed", got, unc, c["C"], xfmax, unc_dts)
    # a (layer, geometry) pair the sequence does not cross, or whose geometry names no path, is exactly zero
    touched = np.zeros((c["L"], Q), bool)
    touched[np.unique(c["LAYINC"])] = np.any(c["C"] != 0, axis=1)[None, :]
    assert np.all(got[3][:, :, ~touched] == 0.0)
    if dc.is_ground(c["lp"], c["LAYINC"]):
        assert np.all(np.abs(got[2][:, np.any(c["C"] != 0, axis=1)]) > 0)
    else:
        assert np.all(got[2] == 0.0)
    return got


@pytest.mark.parametrize("xfac,ispace,tsurf", [(True, 0, -1.0), (False, 0, 180.0), (True, 1, -1.0), (True, 1, 180.0)])
def test_disc_vs_oracle_and_vs_uncollapsed_route(eng, oracle, xfac, ispace, tsurf):
    """W = 130: three wavenumber tiles, the last with two live lanes; G = 10, S = 3, L = 12, three paths down to the ground mixed
    to one geometry, NVMR = 4, NDUST = 1, igas_map [2, 0, 3], random dTAUCON; with and without xfac; on a wavenumber (ISPACE 0)
    and a wavelength (ISPACE 1) axis; the ground at the bottom layer's temperature (TSURF = -1) and a surface at 180 K with an
    emissivity that rises over the window."""
    c = _case(130)
    assert c["C"].shape == (1, 3) and c["LAYINC"].size == 12
    assert np.ptp(c["SCALE"][:, 1] / c["SCALE"][:, 0]) > 0.01              # ragged columns
    _check_case(eng, oracle, c, xfac=xfac, ispace=ispace, tsurf=tsurf)


@pytest.mark.parametrize("W", [64, 1])
def test_disc_whole_tile_and_single_wavenumber(eng, oracle, W):
    _check_case(eng, oracle, _case(W), tsurf=180.0)


@pytest.mark.parametrize("P", [1, CHUNK + 1])
def test_disc_one_path_and_one_more_than_a_lockstep_chunk(eng, oracle, P):
    _check_case(eng, oracle, _case(130, P=P), tsurf=180.0)


def test_disc_three_geometries_share_a_path(eng, oracle):
    """Q = 3 on four paths: neighbouring geometries share path 1, one weight is negative, the last path is named by no geometry
    (it still gets its SPEC) and the third row is empty (MOD, dTSMOD and dMOD exactly 0); the same matrix as compressed rows"""
    c = _case(130, P=4, Q=3)
    got = _check_case(eng, oracle, c, tsurf=180.0)
    assert got[1][:, 3].min() > 0
    assert np.all(got[0][:, 2] == 0.0) and np.all(got[2][:, 2] == 0.0) and np.all(got[3][..., 2] == 0.0)
    nz = c["C"] != 0
    triple = (np.concatenate([[0], np.cumsum(nz.sum(axis=1))]), np.nonzero(nz)[1], c["C"][nz])
    again = eng.cirsradg_ck_disc(0, c["lp"], c["lt"], c["am"], c["cont"], c["dcont"], NVMR, NPAR, IGAS_MAP, c["LAYINC"], c["SCALE"],
                                 c["EMTEMP"], 180.0, EMISSIVITY=c["emis"], mix=triple, xfac=c["xfac"])
    assert all(np.array_equal(x, y) for x, y in zip(got, again))


def test_disc_sequence_without_ground_agrees_with_the_limb_entry(eng, oracle):
    """Down to layer 3 and up again: the lower boundary contributes nothing, dTSMOD is exactly zero whatever TSURF says, and MOD,
    SPEC and dMOD are within the same bounds of cirsradg_ck_limb on the same paths"""
    c = _case(130, kind="limb")
    got = _check_case(eng, oracle, c, tsurf=180.0)
    assert np.all(got[2] == 0.0)
    lM, lS, ldM = eng.cirsradg_ck_limb(0, c["lp"], c["lt"], c["am"], c["cont"], c["dcont"], NVMR, NPAR, IGAS_MAP, *_as_paths(c), c["C"],
                                       xfac=c["xfac"])
    _compare("cirsradg_ck_limb", got, (lM, lS, np.zeros_like(lM), ldM), c["C"], float(c["xfac"].max()), 0.0)


def test_disc_five_layers_and_lbl_table(eng, oracle):
    """L = 5 on the k-table, and G = 1 on a line-by-line table"""
    _check_case(eng, oracle, _case(130, L=5))
    _check_case(eng, oracle, _case(130, L=5, lbl=True), tsurf=180.0)


def test_disc_without_continuum_gradients(eng, oracle):
    got = _check_case(eng, oracle, _case(130), dcont=None)
    free = [k for k in range(NPAR) if k not in set(IGAS_MAP) | {NVMR}]
    assert np.all(got[3][:, free] == 0.0)


def test_disc_with_one_gas_masked(eng, oracle):
    eng.set_gradient_gases([0, 2], temperature=True)
    try:
        _check_case(eng, oracle, _case(130), gases={0, 2})
    finally:
        eng.set_gradient_gases(None)


def test_disc_with_a_pending_shared_gas_gradient(eng, oracle):
    c = _case(130)
    with_term = _check_case(eng, oracle, c, every_gas=True)
    without = _fused(eng, c)                             # consumed: the next call is without it
    assert not np.array_equal(with_term[3][:, :NVMR], without[3][:, :NVMR])
    assert np.array_equal(with_term[3][:, NVMR:], without[3][:, NVMR:]) and np.array_equal(with_term[0], without[0])


def test_disc_slab_beyond_one_lds_stage(eng, oracle):
    """G = 20, S = 16: the 17 slots of the layer's slab go through LDS in chunks; every parameter, whichever chunk its slot lies
    in, agrees, and the parameters without a slot come with the first chunk"""
    c = _wide_case()
    got = _check_case(eng, oracle, c, tsurf=180.0)
    assert np.all(np.abs(got[3]).max(axis=(0, 2, 3)) > 0)


@pytest.mark.parametrize("G,S", [(32, 3), (27, 5), (20, 31), (32, 31)])
def test_disc_at_the_size_limits(eng, oracle, G, S):
    """The chunk rule at its edges (SIZE_CASES of test_limb_gpu.py; the restated slab_chunk keeps each case on its edge): 32
    g-ordinates, where the waves' columns and one slot are the two-block budget exactly; 31 gases, the 32 slots in 8 chunks of 4
    and in 32 chunks of 1, gas 30 and the temperature on bits 30 and 31 of the mask.  Same references and bounds as every case of
    this file."""
    from test_limb_gpu import assert_size_case
    assert_size_case(G, S)
    got = _check_case(eng, oracle, _wide_case(G, S), tsurf=180.0)
    assert np.all(np.abs(got[3]).max(axis=(0, 2, 3)) > 0)


def test_disc_more_geometries_than_waves(eng, oracle):
    """P = 9 averaging points mixed to Q = 9 geometries by rows of two or three weights, row 4 empty: the 8 geometries with a weight
    have an entry in every layer, so every wave of the block serves two and fills its LDS columns again for the second"""
    c = _case(130, P=9, Q=9)
    n = (c["C"] != 0).sum(axis=1)
    assert c["C"].shape == (9, 9) and n[4] == 0 and set(np.delete(n, 4)) == {2, 3} and np.count_nonzero(n) >= 6
    got = _check_case(eng, oracle, c, tsurf=180.0)
    assert np.all(got[0][:, 4] == 0.0) and np.all(got[2][:, 4] == 0.0) and np.all(got[3][..., 4] == 0.0)


def test_disc_conditions(eng, oracle):
    """Equal inputs, equal bits; an un-collapsed call before and after a fused call returns equal bits (no scratch of the one is
    the other's); the scratch beyond the gas stage and dMOD is exactly what include/ansfm.h states, with its formula for the
    g-groups; the kernel times are positive."""
    c = _case(130)
    _upload(eng, c)
    unc = lambda: _thermal(eng, c, c["dcont"], tsurf=180.0)
    before = unc()
    a = _fused(eng, c, tsurf=180.0)
    scratch, ms_sens, ms_grad = eng.disc_last()
    b = _fused(eng, c, tsurf=180.0)
    after = unc()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    (Q, P), G, Wpad, W, L = c["C"].shape, 10, 192, 130, c["L"]
    NT = np.unique(c["EMTEMP"]).size
    GS = min(G, max(4, -(-256 // ((Wpad // 64) * Q))))
    assert GS == 10                                       # 3 tiles x 1 row: every g-ordinate has its own group
    stated = 8 * Wpad * (Q * L * (G + GS) + (P + Q) * G + 2 * (NT + 1)) + 8 * W * (2 * Q + P)
    print("scratch %d bytes (dMOD %d), k_disc_planck + k_disc_sens %.3f ms, k_disc_grad %.3f ms" % (scratch, a[3].nbytes, ms_sens, ms_grad))
    assert scratch == stated
    assert ms_sens > 0 and ms_grad > 0
    # at the shape the design names (W 1024, G 20, Q 1): 16 tiles -> 16 groups, 256 blocks
    assert min(20, max(4, -(-256 // (16 * 1)))) == 16


def test_disc_last_survives_calls_of_the_other_fused_routes(eng, oracle):
    """transit, occultation and limb keep records of their own: after table uploads and one call of each on the same engine,
    disc_last still returns what it returned right after the disc call -- the scratch bytes and, because the entry reads the
    times between its events once when the call ends and keeps them with the record, the same two times"""
    import test_limb_gpu as tlg
    import test_occultation_gpu as tog
    import test_transit_gpu as ttg
    c = _case(130)
    _upload(eng, c)
    _fused(eng, c)
    mine = eng.disc_last()
    for case, call in ((_transit_case(130), ttg._fused), (tog._case(130), tog._fused), (tlg._case(130), tlg._fused)):
        _upload(eng, case)
        call(eng, case)
    again = eng.disc_last()
    assert again[0] == mine[0] > 0
    assert again[1:] == mine[1:] and mine[1] > 0 and mine[2] > 0
    assert eng.disc_last() == mine                       # and asking twice changes nothing


def test_disc_layer_cap_and_invalid_arguments(eng, oracle):
    """L = 160 (the whole 160 KiB of LDS in k_disc_sens) runs and agrees with the un-collapsed route; L = 161 is
    NotImplementedError; TSURF > 0 without EMISSIVITY, a LAYINC outside the layers, an empty sequence, no path and mix entries
    that leave the paths are ValueError."""
    c = _case(64, L=CAP)
    _upload(eng, c)
    got = _fused(eng, c, tsurf=180.0)
    unc, dts_max = _uncollapsed_on_engine(eng, c, np.array(c["dcont"]), tsurf=180.0)
    _compare("L = 160, same engine, un-collapsed", got, unc, c["C"], float(c["xfac"].max()), dts_max)
    with pytest.raises(NotImplementedError):
        _fused(eng, _case(64, L=CAP + 1))
    small = _case(64)
    _upload(eng, small)
    P = small["C"].shape[1]
    args = [0, small["lp"], small["lt"], small["am"], small["cont"], None, NVMR, NPAR, IGAS_MAP]
    call = lambda layinc, scale, emtemp, tsurf, mix, emis=None: eng.cirsradg_ck_disc(*args, layinc, scale, emtemp, tsurf, EMISSIVITY=emis,
                                                                                    mix=mix)
    ok = call(small["LAYINC"], small["SCALE"], small["EMTEMP"], 180.0, small["C"], small["emis"])
    assert np.all(np.isfinite(ok[0]))
    with pytest.raises(ValueError):
        call(small["LAYINC"], small["SCALE"], small["EMTEMP"], 180.0, small["C"])                  # TSURF > 0, no EMISSIVITY
    for bad_layer in (small["L"], -1):
        bad = np.array(small["LAYINC"]); bad[1] = bad_layer
        with pytest.raises(ValueError):
            call(bad, small["SCALE"], small["EMTEMP"], -1.0, small["C"])
    with pytest.raises(ValueError):
        call(small["LAYINC"][:0], small["SCALE"][:0], small["EMTEMP"][:0], -1.0, small["C"])       # N = 0
    with pytest.raises(ValueError):
        call(small["LAYINC"], small["SCALE"][:, :0], small["EMTEMP"], -1.0, np.zeros((1, 0)))      # P = 0
    with pytest.raises(ValueError):
        call(small["LAYINC"], small["SCALE"], small["EMTEMP"], -1.0, (np.array([0, 2]), np.array([0, P]), np.ones(2)))
    with pytest.raises(ValueError):
        call(small["LAYINC"], small["SCALE"], small["EMTEMP"], -1.0, (np.array([0, 2]), np.array([0, -1]), np.ones(2)))
    with pytest.raises(ValueError):
        call(small["LAYINC"], small["SCALE"], small["EMTEMP"], -1.0, (np.array([0, 2, 1]), np.array([0, 1]), np.ones(2)))   # backwards
    with pytest.raises(ValueError):
        call(small["LAYINC"], small["SCALE"], small["EMTEMP"], -1.0, (np.array([1, 2]), np.array([0, 1]), np.ones(2)))      # starts at 1


def test_disc_chain_to_the_state_vector_on_the_device(eng, oracle):
    """map2pro(None) / map2xvec(None) with NPATH = 1 continue from the dMOD the fused call left on the device: the same as the
    oracle's maps of the returned dMOD, within the map tests' 1e-13 of the slot's largest element."""
    c = _case(130)
    _upload(eng, c)
    W, L, Q = c["W"], c["L"], 1
    rng = np.random.default_rng(3)
    NPRO, NX = 17, 9
    DTE, DAM, DCO = (rng.uniform(0, 1, (L, NPRO)) for _ in range(3))
    xmap = rng.normal(size=(NX, NPAR, NPRO))
    nlayin, layinc = np.array([L] * Q), np.ascontiguousarray(np.tile(np.arange(L)[:, None], (1, Q)))
    host = _fused(eng, c)
    with pytest.raises(ValueError):
        eng.map2pro(None, W, NVMR, NDUST, NPRO, Q, nlayin, layinc, DTE, DAM, DCO)       # nothing was left to chain
    dev = _fused(eng, c, gradients_on_device=True)
    assert dev[3] is None and all(np.array_equal(dev[i], host[i]) for i in range(3))
    eng.map2pro(None, W, NVMR, NDUST, NPRO, Q, nlayin, layinc, DTE, DAM, DCO, to_host=False)
    xv = eng.map2xvec(None, W, NVMR, NDUST, NPRO, Q, NX, xmap)
    pro_o = oracle.map2pro(host[3], W, NVMR, NDUST, NPRO, Q, nlayin, layinc, DTE, DAM, DCO)
    xv_o = oracle.map2xvec(pro_o, W, NVMR, NDUST, NPRO, Q, NX, xmap)
    np.testing.assert_allclose(xv, xv_o, rtol=0, atol=1e-13 * np.max(np.abs(xv_o)))


@pytest.mark.parametrize("case", ["", "S_"])
def test_disc_golden_c1(eng, oracle, golden_dir, case):
    """The reference's nemesisdiscfmg on the cut C1 case (three averaging points at 0 / 40 / 65 degrees, weights 0.2 / 0.5 / 0.3)
    through the real engine and the device chain, without a surface (TSURF = 0: the ground at the bottom layer's temperature) and,
    case "S_", with a surface at 180 K and a rising emissivity.  SPEC rtol 2e-7 (float32 table grids); every non-zero column of
    dSPEC within max(16 x the fixture's restatement error, 1e-10) of its largest element plus the derived allowance for the
    cancellation in T_{j-1} - T_j and the rounding of T_end (dc.cancellation_terms, surface terms included); the columns the
    reference leaves zero exactly zero; sum WGEOM dTSURF of the fixture against dTSMOD by the same rule.

    The rule as the issue wrote it does not hold on this case: it asks that the bound so derived stay <= 1e-4, and for the
    topmost temperature level it comes to 1.43e-4 (7.8e-5 for the level below; the vertical paths are thinnest there -- the limb
    fixture's longer paths gave 3.8e-5).  The test therefore holds every column to min(derived bound, 1e-4): no column may be off
    by more than the Jacobian contract of 1e-4, whatever its derived bound says.  Measured: SPEC 4.4e-16; the columns use at most
    5.9 % of their bound; the topmost temperature level 3.4e-6 of its largest element; sum WGEOM dTSURF 4.9e-16 / 7.0e-16."""
    z = np.load(os.path.join(golden_dir, "disc_c1.npz"))
    g = lambda k: z[case + k] if case + k in z.files else z[k]
    eng.upload_ktable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"], z["DELG"])
    L = z["LAY_PRESS"].size
    nvmr, ndust, npro = int(z["NVMR"]), int(z["NDUST"]), int(z["NPRO"])
    npar = nvmr + 2 + ndust
    tsurf = float(g("TSURF"))
    assert (tsurf > 0) == (case == "S_")
    from archnemesis_dist_amd import disc
    C = disc.average_mix(z["WGEOM"])
    amount = np.ascontiguousarray(z["LAY_AMOUNT"].T) * 1.0e-4
    MOD, SPEC, dTSMOD, dMOD = eng.cirsradg_ck_disc(int(z["ISPACE"]), z["LAY_PRESS"], z["LAY_TEMP"], amount, z["TAUCONT"], z["dTAUCON"], nvmr,
                                                   npar, z["igas_map"], z["LAYINC"], z["SCALE"], z["EMTEMP"], tsurf,
                                                   EMISSIVITY=g("EMISSIVITY") if tsurf > 0 else None, mix=C, xfac=z["XFAC"],
                                                   gradients_on_device=True)
    assert dMOD is None
    W, NX = MOD.shape[0], z["xmap"].shape[0]
    eng.map2pro(None, W, nvmr, ndust, npro, 1, np.array([L]), np.arange(L)[:, None], z["DTE"], z["DAM"], z["DCO"],
                INCPAR=list(z["incpar"]), to_host=False)
    dspec = eng.map2xvec(None, W, nvmr, ndust, npro, 1, NX, z["xmap"])[:, 0, :]          # (W, NX)
    assert int(z["JSURF"]) < 0                          # no surface-temperature element in this state vector: no column replaced
    ref = g("dSPEC")
    scale = np.abs(ref).max(axis=0)
    nonzero = scale > 0
    assert np.count_nonzero(nonzero) >= 60
    err = np.abs(dspec - ref).max(axis=0) / np.where(nonzero, scale, 1.0)
    by_col, for_ts = dc.golden_cancellation_by_column(z, oracle, case)
    cancel = 4.0 * 2.0 ** -53 * by_col
    derived = np.maximum(16.0 * g("restatement_err"), 1e-10) + cancel
    # never beyond the Jacobian contract of 1e-4, whatever the derived bound of a column is (see the docstring)
    bound = np.minimum(derived, 1e-4)
    print("columns by err / bound:", np.array2string((err / bound)[nonzero], precision=2))
    print("SPEC rel %.3e; worst column %.3e of its largest element (bound there %.3e); worst err / bound %.3e; largest derived bound %.3e"
          % (np.max(np.abs(MOD[:, 0] / g("SPEC") - 1.0)), err[nonzero].max(), bound[np.argmax(np.where(nonzero, err, 0.0))],
             np.max((err / bound)[nonzero]), derived.max()))
    assert bound.shape == (NX,) and bound.max() <= 1e-4
    np.testing.assert_allclose(MOD[:, 0], g("SPEC"), rtol=2e-7)
    np.testing.assert_allclose(SPEC * z["XFAC"][:, None], g("SPECOUT"), rtol=2e-7)
    assert np.all(err[nonzero] <= bound[nonzero])
    assert np.all(dspec[:, ~nonzero] == 0.0)
    ts_ref = g("dTSURF") @ np.asarray(z["WGEOM"], dtype=np.float64)
    ts_bound = max(16.0 * float(g("restatement_err_dtsurf")), 1e-10) + 4.0 * 2.0 ** -53 * for_ts
    ts_err = np.abs(dTSMOD[:, 0] - ts_ref).max() / np.abs(ts_ref).max()
    print("sum WGEOM dTSURF: %.3e of its largest element (bound %.3e)" % (ts_err, ts_bound))
    assert ts_bound <= 1e-4 and ts_err <= ts_bound
