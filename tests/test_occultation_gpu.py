"""ansfm_cirsradg_ck_occultation on the GPU (k_occ_paths, k_occ_grad): the limb paths of a solar occultation mixed to the
geometries of the measurement with their layer gradients, against the collapsed restatement (tests/occultation_cases.py) on the
CPU oracle's opacities, against the un-collapsed route of the same engine (cirsradg_ck_transmission, then the restatement's
mix), against cirsradg_ck_transit where the mix is one row of annulus weights, and against the reference's nemesisSOfmg in
tests/golden/occultation_c1.npz.

Tolerances are those of test_transit_gpu / test_cirsradg_transmission_vs_oracle for this branch: 1e-11 relative on a
transmission, 1e-10 of the parameter slab's largest element on a gradient.  MOD[w, q] = xfac sum_p C[q, p] T_p with T_p <= 1
inherits 1e-11 max|xfac| sum_p |C[q, p]|."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occultation_cases as oc  # noqa: E402
import transit_cases as tc  # noqa: E402
from test_transit_gpu import _case as _transit_case  # noqa: E402  (the synthetic generator: G = 10, S = 3, or G = 1 on an LBL table)

pytestmark = pytest.mark.gpu

NVMR, NDUST = 4, 1
NPAR = NVMR + 2 + NDUST
IGAS_MAP = np.array([2, 0, 3], dtype=np.int32)
CAP = 320                       # layers / paths of the fused call (include/ansfm.h)


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


@functools.lru_cache(maxsize=None)
def _case(W, L=12, lbl=False, kind="pairs"):
    """A case of test_transit_gpu._case with some of its limb paths (path p runs down to layer p and up again) and a mixing
    matrix.  pairs: Q = 3 geometries on 6 bracketing paths, two entries a row (L = 5: Q = 2 on 4 paths).  general: all L - 1
    paths, C (5, L - 1) with dense rows, negative entries, an empty row and a row that names the last path only.  transit:
    all paths, one row of annulus weights.  cap: 4 paths, Q = 2."""
    t = _transit_case(W, L, lbl)
    rng = np.random.default_rng(5 + W + 1000 * L)
    P0 = L - 1
    if kind == "pairs":
        keep = np.array([1, 2, 5, 6, 8, 9]) if L >= 12 else np.array([0, 1, 2, 3])
        Q = keep.size // 2
        C = np.zeros((Q, keep.size))
        for q in range(Q):
            f = rng.uniform(0.1, 0.9)
            C[q, 2 * q], C[q, 2 * q + 1] = 1.0 - f, f
    elif kind == "general":
        keep = np.arange(P0)
        C = np.zeros((5, P0))
        C[0] = rng.uniform(0.1, 1.0, P0)
        C[1] = rng.uniform(-1.0, 1.0, P0)
        C[3, P0 - 1] = 0.75                                   # row 2 stays empty
        C[4, [0, 3, 4]] = [-0.5, 2.0, 0.25]
    elif kind == "transit":
        keep = np.arange(P0)
        C = np.array(t["weight"])[None, :]
    elif kind == "many":
        from test_limb_gpu import many_geometries
        keep, C = np.arange(P0), many_geometries(P0, rng)
    else:                                                     # cap
        keep = np.linspace(0, L - 2, 4).astype(int)
        C = np.array([[0.3, 0.7, 0.0, 0.0], [0.0, 0.0, 0.6, 0.4]])
    c = {k: v for k, v in t.items() if k not in ("NLAYIN", "LAYINC", "SCALE", "weight")}
    c["NLAYIN"] = np.ascontiguousarray(t["NLAYIN"][keep])
    c["LAYINC"] = np.ascontiguousarray(t["LAYINC"][:, keep])
    c["SCALE"] = np.ascontiguousarray(t["SCALE"][:, keep])
    c["C"] = C
    c["xfac"] = rng.uniform(0.5, 2.0, W) * 1.0e3
    c["G"] = 1 if lbl else 10
    return _freeze(c)


def _wide_case(G=20, S=16):
    """test_limb_gpu._wide_case (L = 4, W = 64; G = 20, S = 16: 17 slots of 10 KiB beside 40 KiB of columns, more than one LDS
    stage holds) drawn from this file's seed and without EMTEMP"""
    from test_limb_gpu import _wide_case as limb_wide_case
    return limb_wide_case(G, S, "two", seed=91, emtemp=False)


_ORACLE = {}


def _opacities(oracle, c):
    """tautot (W, G, L) and the gradient merge's dk (W, G, L, S + 1) of a case by the CPU oracle, once.  The key names everything
    a generator's arrays depend on: two cases that differ in G or in the generator's seed alone do not share an entry."""
    key = (c["W"], c["L"], c["lbl"], c["S"], c["G"], c.get("tag"))
    if key not in _ORACLE:
        if c["lbl"]:
            k, dkdT = oracle.calc_klbl(c["K"], c["PRESS"], c["TEMP"], c["lp"] / 101325.0, c["lt"], grad=True)       # (W, L, S)
            tau = np.einsum("wls,sl->wl", k, c["am"])[:, None, :]
            dk = np.concatenate([k, np.einsum("wls,sl->wl", dkdT, c["am"])[:, :, None]], axis=2)[:, None, :, :]
        else:
            k, dkdT = oracle.calc_k(c["K"], c["PRESS"], c["TEMP"], c["lp"] / 101325.0, c["lt"], grad=True)
            tau, dk = oracle.k_overlapg(c["delg"], k, dkdT, c["am"])
        _ORACLE[key] = (tau + c["cont"][:, None, :], dk)
    return _ORACLE[key]


def _upload(eng, c):
    if c["lbl"]:
        eng.upload_lbltable(c["K"], c["PRESS"], c["TEMP"], c["WAVE"])
    else:
        eng.upload_ktable(c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"])


def _dims(c):
    return c.get("NVMR", NVMR), c.get("NPAR", NPAR), c.get("igas_map", IGAS_MAP)


def _fused(eng, c, dcont="dcont", xfac=True, **kw):
    nvmr, npar, ig = _dims(c)
    return eng.cirsradg_ck_occultation(c["lp"], c["lt"], c["am"], c["cont"], None if dcont is None else c[dcont], nvmr, npar, ig,
                                       c["NLAYIN"], c["LAYINC"], c["SCALE"], c["C"], xfac=c["xfac"] if xfac else None, **kw)


def _uncollapsed_on_engine(eng, c, dcont, xfac=True):
    nvmr, npar, ig = _dims(c)
    spec, dspec = eng.cirsradg_ck_transmission(c["lp"], c["lt"], c["am"], c["cont"], dcont, nvmr, npar, ig, c["NLAYIN"],
                                               c["LAYINC"], c["SCALE"], xfac=c["xfac"] if xfac else None)
    MOD, dMOD = oc.mod_from_paths(spec, dspec, c["C"], c["NLAYIN"], c["LAYINC"], c["L"])
    return MOD, spec / (c["xfac"][:, None] if xfac else 1.0), dMOD


def _compare(what, got, ref, C, xfmax, trans_rtol=1e-11):
    (MOD, TRANS, dMOD), (rM, rT, rdM) = got, ref
    scale = np.max(np.abs(rdM), axis=(0, 2, 3), keepdims=True)
    err = np.max(np.abs(dMOD - rdM) / np.where(scale > 0, scale, 1.0), axis=(0, 2, 3))
    atol = 1e-11 * xfmax * np.abs(C).sum(axis=1)
    print("%s: TRANS rel %.3e, MOD / its bound %.3e, dMOD by parameter %s" % (
        what, np.max(np.abs(TRANS - rT) / rT), np.max(np.abs(MOD - rM) / np.where(atol > 0, atol, 1.0)[None, :]),
        np.array2string(err, precision=2)))
    np.testing.assert_allclose(TRANS, rT, rtol=trans_rtol)
    assert np.all(np.abs(MOD - rM) <= atol[None, :])
    assert err.max() < 1e-10
    assert np.all(dMOD[:, scale.reshape(-1) == 0] == 0.0)


def _check_case(eng, oracle, c, dcont="dcont", xfac=True, gases=None, temperature=True, every_gas=False):
    nvmr, npar, ig = _dims(c)
    _upload(eng, c)
    got = _fused(eng, c, dcont, xfac, dtau_every_gas=c["dray"] if every_gas else None)
    Q, P = c["C"].shape
    assert got[0].shape == (c["W"], Q) and got[1].shape == (c["W"], P) and got[2].shape == (c["W"], npar, c["L"], Q)
    tautot, dk = _opacities(oracle, c)
    dtau = tc.dtautot(dk, ig, nvmr, npar, None if dcont is None else c[dcont], c["dray"] if every_gas else None,
                      gases=gases, temperature=temperature)
    Sm = tc.path_matrix(c["L"], c["NLAYIN"], c["LAYINC"], c["SCALE"])
    xf = c["xfac"] if xfac else None
    ref = oc.collapsed(tautot, np.asarray(c["delg"], dtype=np.float64), Sm, c["C"], dtau, xf)
    assert np.abs(ref[2]).max() > 0 and ref[1].min() > 1e-200 and ref[1].max() < 1.0 + 1e-6
    xfmax = float(np.abs(c["xfac"]).max()) if xfac else 1.0
    _compare("oracle, collapsed", got, ref, c["C"], xfmax)
    dc = None if dcont is None else np.array(c[dcont])
    if every_gas:                                        # the un-collapsed call takes the shared term inside dtaucon
        dc = np.zeros((c["W"], npar, c["L"])) if dc is None else dc
        dc[:, :nvmr, :] += c["dray"][:, None, :]
    _compare("same engine, un-collapsed", got, _uncollapsed_on_engine(eng, c, dc, xfac), c["C"], xfmax)
    # a (layer, geometry) pair no path of the geometry crosses is exactly zero
    touched = (Sm != 0.0).astype(float) @ (c["C"] != 0.0).T.astype(float) > 0          # (L, Q)
    assert np.all(got[2][:, :, ~touched] == 0.0)
    return got


@pytest.mark.parametrize("xfac", [True, False])
def test_occultation_vs_oracle_and_vs_uncollapsed_route(eng, oracle, xfac):
    """W = 130: three wavenumber tiles, the last with two live lanes; G = 10, S = 3, L = 12, Q = 3 geometries on the 6 limb paths
    that bracket them (two entries a row), NVMR = 4, NDUST = 1, igas_map [2, 0, 3], random dTAUCON; with and without xfac."""
    c = _case(130)
    assert c["C"].shape == (3, 6) and np.all((c["C"] != 0).sum(axis=1) == 2)
    _check_case(eng, oracle, c, xfac=xfac)


@pytest.mark.parametrize("W", [64, 1])
def test_occultation_whole_tile_and_single_wavenumber(eng, oracle, W):
    _check_case(eng, oracle, _case(W))


def test_occultation_general_mixing_matrix(eng, oracle):
    """C (5, 11): a dense row, a row with negative entries, an empty row (MOD and dMOD exactly 0), a row that names the last
    path only, a row of three"""
    c = _case(130, kind="general")
    got = _check_case(eng, oracle, c)
    assert np.all(got[0][:, 2] == 0.0) and np.all(got[2][..., 2] == 0.0)
    assert np.array_equal(got[0][:, 3], c["xfac"] * (0.75 * got[1][:, -1]))
    # the same matrix as compressed rows
    nz = c["C"] != 0
    triple = (np.concatenate([[0], np.cumsum(nz.sum(axis=1))]), np.nonzero(nz)[1], c["C"][nz])
    again = eng.cirsradg_ck_occultation(c["lp"], c["lt"], c["am"], c["cont"], c["dcont"], NVMR, NPAR, IGAS_MAP, c["NLAYIN"],
                                        c["LAYINC"], c["SCALE"], triple, xfac=c["xfac"])
    assert all(np.array_equal(x, y) for x, y in zip(got, again))


def test_occultation_on_lbl_table(eng, oracle):
    """G = 1 on a line-by-line table, L = 5"""
    _check_case(eng, oracle, _case(130, L=5, lbl=True))


def test_occultation_without_continuum_gradients(eng, oracle):
    got = _check_case(eng, oracle, _case(130), dcont=None)
    free = [k for k in range(NPAR) if k not in set(IGAS_MAP) | {NVMR}]
    assert np.all(got[2][:, free] == 0.0)


def test_occultation_with_one_gas_masked(eng, oracle):
    eng.set_gradient_gases([0, 2], temperature=True)
    try:
        _check_case(eng, oracle, _case(130), gases={0, 2})
    finally:
        eng.set_gradient_gases(None)


def test_occultation_with_a_pending_shared_gas_gradient(eng, oracle):
    c = _case(130)
    with_term = _check_case(eng, oracle, c, every_gas=True)
    without = _fused(eng, c)                             # consumed: the next call is without it
    assert not np.array_equal(with_term[2][:, :NVMR], without[2][:, :NVMR])
    assert np.array_equal(with_term[2][:, NVMR:], without[2][:, NVMR:]) and np.array_equal(with_term[0], without[0])


def test_occultation_slab_beyond_one_lds_stage(eng, oracle):
    """G = 20, S = 16: the 17 slots of the layer's slab go through LDS in chunks of 4; every parameter, whichever chunk its slot
    lies in, agrees, and the parameters without a slot come with the first chunk"""
    c = _wide_case()
    got = _check_case(eng, oracle, c)
    assert np.all(np.abs(got[2]).max(axis=(0, 2, 3)) > 0)


@pytest.mark.parametrize("G,S", [(32, 3), (27, 5), (20, 31), (32, 31)])
def test_occultation_at_the_size_limits(eng, oracle, G, S):
    """The chunk rule at its edges (SIZE_CASES of test_limb_gpu.py; the restated slab_chunk keeps each case on its edge): 32
    g-ordinates, where the waves' columns and one slot are the two-block budget exactly; 31 gases, the 32 slots in 8 chunks of 4
    and in 32 chunks of 1, gas 30 and the temperature on bits 30 and 31 of the mask.  Same references and bounds as every case of
    this file."""
    from test_limb_gpu import assert_size_case
    assert_size_case(G, S)
    c = _wide_case(G, S)
    got = _check_case(eng, oracle, c)
    assert np.all(np.abs(got[2]).max(axis=(0, 2, 3)) > 0)


def test_occultation_more_geometries_than_waves(eng, oracle):
    """Q = 9 on the 11 tangent paths (many_geometries of test_limb_gpu.py): in the top layers 8 geometries have an entry and every
    wave of the block serves two, filling its LDS columns again for the second; row 4 is empty."""
    c = _case(130, kind="many")
    Sm = tc.path_matrix(c["L"], c["NLAYIN"], c["LAYINC"], c["SCALE"])
    entries = ((Sm != 0.0).astype(float) @ (c["C"] != 0.0).T.astype(float) > 0).sum(axis=1)          # geometries by layer
    assert c["C"].shape == (9, 11) and entries.max() >= 6 and entries.min() == 1 and not np.any(c["C"][4])
    got = _check_case(eng, oracle, c)
    assert np.all(got[0][:, 4] == 0.0) and np.all(got[2][..., 4] == 0.0)


def test_occultation_with_transit_weights_equals_the_transit_entry(eng, oracle):
    """Q = 1 with C = c, the annulus weights: sum c - MOD is AREA and -dMOD[..., 0] is dAREA of cirsradg_ck_transit.  Different
    kernels, with their sums over paths in a different association: 1e-12 of the largest element, not bit equality."""
    c = _case(130, kind="transit")
    t = _transit_case(130)
    _upload(eng, c)
    MOD, TRANS, dMOD = _fused(eng, c, xfac=False)
    AREA, T2, dAREA = eng.cirsradg_ck_transit(t["lp"], t["lt"], t["am"], t["cont"], t["dcont"], NVMR, NPAR, IGAS_MAP, t["NLAYIN"],
                                              t["LAYINC"], t["SCALE"], t["weight"])
    np.testing.assert_allclose(TRANS, T2, rtol=1e-13)
    area = c["C"].sum() - MOD[:, 0]
    print("AREA %.3e, dAREA %.3e of the largest element" % (np.abs(area - AREA).max() / np.abs(AREA).max(),
                                                           np.abs(-dMOD[..., 0] - dAREA).max() / np.abs(dAREA).max()))
    assert np.abs(area - AREA).max() <= 1e-12 * np.abs(AREA).max()
    assert np.abs(-dMOD[..., 0] - dAREA).max() <= 1e-12 * np.abs(dAREA).max()


def test_occultation_chain_to_the_state_vector_on_the_device(eng, oracle):
    """map2pro(None) / map2xvec(None) with NPATH = Q continue from the dMOD the fused call left on the device: the same as the
    oracle's maps of the returned dMOD, within the map tests' 1e-13 of the slot's largest element."""
    c = _case(130)
    _upload(eng, c)
    W, L, Q = c["W"], c["L"], c["C"].shape[0]
    rng = np.random.default_rng(3)
    NPRO, NX = 17, 9
    DTE, DAM, DCO = (rng.uniform(0, 1, (L, NPRO)) for _ in range(3))
    xmap = rng.normal(size=(NX, NPAR, NPRO))
    nlayin, layinc = np.array([L] * Q), np.ascontiguousarray(np.tile(np.arange(L)[:, None], (1, Q)))
    host = _fused(eng, c)
    with pytest.raises(ValueError):
        eng.map2pro(None, W, NVMR, NDUST, NPRO, Q, nlayin, layinc, DTE, DAM, DCO)       # nothing was left to chain
    dev = _fused(eng, c, gradients_on_device=True)
    assert dev[2] is None and np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])
    pro = eng.map2pro(None, W, NVMR, NDUST, NPRO, Q, nlayin, layinc, DTE, DAM, DCO)
    assert eng.map2pro(None, W, NVMR, NDUST, NPRO, Q, nlayin, layinc, DTE, DAM, DCO, to_host=False) is None
    xv = eng.map2xvec(None, W, NVMR, NDUST, NPRO, Q, NX, xmap)
    pro_o = oracle.map2pro(host[2], W, NVMR, NDUST, NPRO, Q, nlayin, layinc, DTE, DAM, DCO)
    xv_o = oracle.map2xvec(pro_o, W, NVMR, NDUST, NPRO, Q, NX, xmap)
    assert pro.shape == (W, NPAR, NPRO, Q) and xv.shape == (W, Q, NX)
    for par in range(NPAR):
        np.testing.assert_allclose(pro[:, par], pro_o[:, par], rtol=0, atol=1e-13 * np.max(np.abs(pro_o[:, par])))
    np.testing.assert_allclose(xv, xv_o, rtol=0, atol=1e-13 * np.max(np.abs(xv_o)))


def test_occultation_conditions(eng, oracle):
    """Equal inputs, equal bits; an un-collapsed call before and after a fused call returns equal bits (no scratch of the one is
    the other's); the scratch beyond the gas stage and dMOD stays within (P G + P + Q) Wpad doubles: no factor LIMAX P NPAR."""
    c = _case(130)
    _upload(eng, c)
    unc = lambda: eng.cirsradg_ck_transmission(c["lp"], c["lt"], c["am"], c["cont"], c["dcont"], NVMR, NPAR, IGAS_MAP, c["NLAYIN"],
                                               c["LAYINC"], c["SCALE"], xfac=c["xfac"])
    before = unc()
    a = _fused(eng, c)
    scratch, ms_paths, ms_grad = eng.occultation_last()
    b = _fused(eng, c)
    after = unc()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    (Q, P), G, Wpad = c["C"].shape, 10, 192
    bound = (P * G + P + Q) * Wpad * 8
    print("scratch %d bytes (bound %d; dMOD %d), k_occ_paths %.3f ms, k_occ_grad %.3f ms" % (scratch, bound, a[2].nbytes, ms_paths, ms_grad))
    assert 0 < scratch <= bound
    assert ms_paths > 0 and ms_grad > 0


def test_occultation_layer_cap(eng, oracle):
    """L = 320 (the whole 160 KiB tile of the path stage) with P = 4, Q = 2 runs and agrees with the un-collapsed route; L = 321
    is NotImplementedError; paths that leave the layers or the LAYINC rows and mix entries that leave the paths are ValueError;
    padding beyond NLAYIN is never read."""
    c = _case(64, L=CAP, kind="cap")
    _upload(eng, c)
    got = _fused(eng, c)
    _compare("L = 320, same engine, un-collapsed", got, _uncollapsed_on_engine(eng, c, np.array(c["dcont"])), c["C"],
             float(c["xfac"].max()))
    assert got[1].min() > 1e-200
    with pytest.raises(NotImplementedError):
        _fused(eng, _case(64, L=CAP + 1, kind="cap"))
    small = _case(64)
    Q, P = small["C"].shape
    args = [small["lp"], small["lt"], small["am"], small["cont"], None, NVMR, NPAR, IGAS_MAP]
    call = lambda nlayin, layinc, mix: eng.cirsradg_ck_occultation(*args, nlayin, layinc, small["SCALE"], mix)
    bad = np.array(small["LAYINC"]); bad[1, 0] = small["L"]
    with pytest.raises(ValueError):
        call(small["NLAYIN"], bad, small["C"])
    long = np.array(small["NLAYIN"]); long[0] = small["LAYINC"].shape[0] + 1      # more entries than LAYINC has rows
    with pytest.raises(ValueError):
        call(long, small["LAYINC"], small["C"])
    with pytest.raises(ValueError):
        call(small["NLAYIN"], small["LAYINC"], (np.array([0, 1, 2, 3]), np.array([0, P, 1]), np.ones(3)))      # a path that is not there
    with pytest.raises(ValueError):
        call(small["NLAYIN"], small["LAYINC"], (np.array([0, 1, 2, 3]), np.array([0, -1, 1]), np.ones(3)))
    with pytest.raises(ValueError):
        call(small["NLAYIN"], small["LAYINC"], (np.array([0, 2, 1, 3]), np.array([0, 1, 2]), np.ones(3)))      # rows that run backwards
    pads = np.array(small["LAYINC"]); pads[-1, 5] = 10 ** 6            # beyond NLAYIN[5]: padding, never read
    ok = call(small["NLAYIN"], pads, small["C"])
    ref = call(small["NLAYIN"], small["LAYINC"], small["C"])
    assert all(np.array_equal(x, y) for x, y in zip(ok, ref))


def test_occultation_golden_c1(eng, oracle, golden_dir):
    """The reference's nemesisSOfmg on the cut C1 case (three tangent heights on six bracketing paths) through the real engine
    and the device chain: SPECMOD rtol 2e-7 (float32 table grids), every non-zero column of dSPECMOD within
    max(16 x the fixture's restatement error, 1e-10) of its largest element -- a bound that stays below the 1e-4 contract --
    and the columns the reference leaves zero exactly zero."""
    from archnemesis_dist_amd import occultation
    z = np.load(os.path.join(golden_dir, "occultation_c1.npz"))
    eng.upload_ktable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"], z["DELG"])
    L = z["LAY_PRESS"].size
    nvmr, ndust, npro = int(z["NVMR"]), int(z["NDUST"]), int(z["NPRO"])
    npar = nvmr + 2 + ndust
    tan = occultation.tangent_heights_km(z["BASEH"], z["NLAYIN"], z["LAYINC"])
    C = occultation.tangent_mix(tan, z["TANHE"])
    Q = C.shape[0]
    amount = np.ascontiguousarray(z["LAY_AMOUNT"].T) * 1.0e-4
    MOD, TRANS, dMOD = eng.cirsradg_ck_occultation(z["LAY_PRESS"], z["LAY_TEMP"], amount, z["TAUCONT"], z["dTAUCON"], nvmr, npar,
                                                   z["igas_map"], z["NLAYIN"], z["LAYINC"], z["SCALE"], C, xfac=z["XFAC"],
                                                   gradients_on_device=True)
    assert dMOD is None
    W, NX = MOD.shape[0], z["xmap"].shape[0]
    eng.map2pro(None, W, nvmr, ndust, npro, Q, np.array([L] * Q), np.tile(np.arange(L)[:, None], (1, Q)), z["DTE"], z["DAM"], z["DCO"],
                INCPAR=list(z["incpar"]), to_host=False)
    dspec = eng.map2xvec(None, W, nvmr, ndust, npro, Q, NX, z["xmap"])          # (W, Q, NX)
    ref = z["dSPECMOD"]
    scale = np.abs(ref).max(axis=(0, 1))                                        # (NX,): a column over wavenumbers and geometries
    nonzero = scale > 0
    assert np.count_nonzero(nonzero) == 63 and np.count_nonzero(~nonzero) == 18
    err = np.abs(dspec - ref).max(axis=(0, 1)) / np.where(nonzero, scale, 1.0)
    bound = np.maximum(16.0 * z["restatement_err"], 1e-10)
    print("SPECMOD rel %.3e; worst column %.3e of its largest element (bound there %.3e); worst err / bound %.3e"
          % (np.max(np.abs(MOD / z["SPECMOD"] - 1.0)), err[nonzero].max(), bound[np.argmax(np.where(nonzero, err, 0.0))],
             np.max((err / bound)[nonzero])))
    assert bound.shape == (NX,) and bound.max() <= 1e-4
    np.testing.assert_allclose(MOD, z["SPECMOD"], rtol=2e-7)
    assert np.all(err[nonzero] <= bound[nonzero])
    assert np.all(dspec[:, :, ~nonzero] == 0.0)
