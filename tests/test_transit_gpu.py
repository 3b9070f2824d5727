"""ansfm_cirsradg_ck_transit on the GPU (k_transit_sens, k_transit_grad): the transit depth and its layer gradients collapsed
over the limb paths, against the collapsed restatement (tests/transit_cases.py) on the CPU oracle's opacities, against the
un-collapsed route of the same engine (cirsradg_ck_transmission, then the restatement's trapezoid), and against the
reference's nemesisPTfm(gradients=True) in tests/golden/transit_c1.npz.

Tolerances are those of test_cirsradg_transmission_vs_oracle for this branch: 1e-11 relative on a transmission, 1e-10 of the
parameter slab's largest element on a gradient.  AREA = sum_p c_p (1 - T_p) with T_p <= 1 inherits 1e-11 sum_p c_p."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transit_cases as tc  # noqa: E402

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


@functools.lru_cache(maxsize=None)
def _case(W, L=12, lbl=False, P=None):
    """Inputs of one synthetic case (G = 10, S = 3 on a k-table; G = 1 on an LBL table) and nothing of the engine; arrays are
    shared between tests and never written."""
    from archnemesis_dist_amd import synthetic as syn
    rng = np.random.default_rng(78 + W + 1000 * L)
    S = 3
    c = dict(W=W, L=L, S=S, lbl=lbl)
    if lbl:
        NP, NT = 7, 6
        c["PRESS"] = np.logspace(-6, 1.1, NP); c["TEMP"] = np.linspace(80.0, 420.0, NT)
        c["K"] = 10.0 ** rng.uniform(-27, -21, size=(W, NP, NT, S))
        c["WAVE"] = 2500.0 + 0.005 * np.arange(W)
        c["delg"] = np.array([1.0])
        c["lp"] = np.logspace(4.0, 1.0, L); c["lt"] = np.linspace(230.0, 150.0, L)
        c["am"] = 10.0 ** rng.uniform(20.5, 22.0, (S, 1)) * (c["lp"][None, :] / c["lp"][0])
    else:
        c["PRESS"], c["TEMP"], c["K"] = syn.synth_ktable(W, 10, 8, 6, S, seed=22)
        c["delg"] = syn.gauss_legendre_01(10)[1]
        c["WAVE"] = 900.0 + 0.7 * np.arange(W)
        c["lp"] = np.logspace(4.5, 0.5, L); c["lt"] = np.linspace(200, 140, L)
        c["am"] = 10.0 ** rng.uniform(17, 19.5, (S, L)) * (c["lp"][None, :] / c["lp"][:1]) * (12.0 / L)
    c["cont"] = 10.0 ** rng.uniform(-4, -1, (W, L)) * (12.0 / L)
    c["dcont"] = 10.0 ** rng.uniform(-24, -22, (W, NPAR, L))
    c["dray"] = 10.0 ** rng.uniform(-24, -22, (W, L))
    NLAYIN, LAYINC, SCALE = tc.limb_paths(L, rng)
    if P is not None:                                   # a few of the limb paths only
        keep = np.linspace(0, L - 2, P).astype(int)
        NLAYIN, LAYINC, SCALE = NLAYIN[keep], LAYINC[:, keep], SCALE[:, keep]
    c["NLAYIN"], c["LAYINC"], c["SCALE"] = NLAYIN, np.ascontiguousarray(LAYINC), np.ascontiguousarray(SCALE)
    c["weight"] = rng.uniform(1e9, 1e11, NLAYIN.size)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return c


@functools.lru_cache(maxsize=None)
def _wide_case(G=20, S=16):
    """test_limb_gpu._wide_case (L = 4, W = 64, NVMR = S + 2, the 3 limb paths; the amounts of a size case scaled as there) drawn
    from this file's seed, without EMTEMP and the mix, with annulus weights"""
    from test_limb_gpu import _wide_case as limb_wide_case
    c = {k: v for k, v in limb_wide_case(G, S, "two", seed=90, emtemp=False).items() if k not in ("C", "xfac")}
    c["weight"] = np.random.default_rng(90).uniform(1e9, 1e11, c["NLAYIN"].size)
    c["weight"].flags.writeable = False
    return c


_ORACLE = {}


def _opacities(oracle, c):
    """tautot (W, G, L) and the gradient merge's dk (W, G, L, S + 1) of a case by the CPU oracle, once.  The key names everything
    a generator's arrays depend on: two cases that differ in S, in G or in the generator's seed alone do not share an entry."""
    key = (c["W"], c["L"], c["lbl"], c["S"], c.get("G"), c.get("tag"))
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


def _fused(eng, c, dcont="dcont", **kw):
    nvmr, npar, ig = _dims(c)
    return eng.cirsradg_ck_transit(c["lp"], c["lt"], c["am"], c["cont"], None if dcont is None else c[dcont], nvmr, npar, ig,
                                   c["NLAYIN"], c["LAYINC"], c["SCALE"], c["weight"], **kw)


def _uncollapsed_on_engine(eng, c, dcont):
    nvmr, npar, ig = _dims(c)
    spec, dspec = eng.cirsradg_ck_transmission(c["lp"], c["lt"], c["am"], c["cont"], dcont, nvmr, npar, ig, c["NLAYIN"],
                                               c["LAYINC"], c["SCALE"])
    AREA, dAREA = tc.area_from_paths(spec, dspec, c["weight"], c["NLAYIN"], c["LAYINC"], c["L"])
    return AREA, spec, dAREA


def _compare(what, got, ref, weight):
    (AREA, TRANS, dAREA), (rA, rT, rdA) = got, ref
    scale = np.max(np.abs(rdA), axis=(0, 2), keepdims=True)
    err = np.max(np.abs(dAREA - rdA) / np.where(scale > 0, scale, 1.0), axis=(0, 2))
    print("%s: TRANS rel %.3e, AREA / sum c %.3e, dAREA by parameter %s" % (
        what, np.max(np.abs(TRANS - rT) / rT), np.max(np.abs(AREA - rA)) / weight.sum(), np.array2string(err, precision=2)))
    np.testing.assert_allclose(TRANS, rT, rtol=1e-11)
    np.testing.assert_allclose(AREA, rA, rtol=0, atol=1e-11 * weight.sum())
    assert err.max() < 1e-10
    assert np.all(dAREA[:, scale.reshape(-1) == 0, :] == 0.0)


def _check_case(eng, oracle, c, dcont="dcont", gases=None, temperature=True, every_gas=False):
    nvmr, npar, ig = _dims(c)
    _upload(eng, c)
    got = _fused(eng, c, dcont, dtau_every_gas=c["dray"] if every_gas else None)
    assert got[0].shape == (c["W"],) and got[1].shape == (c["W"], c["NLAYIN"].size) and got[2].shape == (c["W"], npar, c["L"])
    tautot, dk = _opacities(oracle, c)
    dtau = tc.dtautot(dk, ig, nvmr, npar, None if dcont is None else c[dcont], c["dray"] if every_gas else None,
                      gases=gases, temperature=temperature)
    Sm = tc.path_matrix(c["L"], c["NLAYIN"], c["LAYINC"], c["SCALE"])
    ref = tc.collapsed(tautot, np.asarray(c["delg"], dtype=np.float64), Sm, c["weight"], dtau)
    assert np.abs(ref[2]).max() > 0 and ref[1].min() > 1e-200 and ref[1].max() < 1.0 + 1e-6
    _compare("oracle, collapsed", got, ref, c["weight"])
    dc = None if dcont is None else np.array(c[dcont])
    if every_gas:                                        # the un-collapsed call takes the shared term inside dtaucon
        dc = np.zeros((c["W"], npar, c["L"])) if dc is None else dc
        dc[:, :nvmr, :] += c["dray"][:, None, :]
    _compare("same engine, un-collapsed", got, _uncollapsed_on_engine(eng, c, dc), c["weight"])
    return got


def test_transit_vs_oracle_and_vs_uncollapsed_route(eng, oracle):
    """W = 130: three wavenumber tiles, the last with two live lanes; G = 10, S = 3, L = 12, P = 11 limb paths as calc_path_PT
    makes them (SCALE in [1, 30] inside, 0 outside), NVMR = 4, NDUST = 1, igas_map [2, 0, 3], random dTAUCON and weights."""
    c = _case(130)
    assert c["NLAYIN"].size == 11 and np.array_equal(c["NLAYIN"], 2 * (12 - np.arange(11)))
    _check_case(eng, oracle, c)


@pytest.mark.parametrize("W", [64, 1])
def test_transit_whole_tile_and_single_wavenumber(eng, oracle, W):
    _check_case(eng, oracle, _case(W))


def test_transit_slab_of_seventeen_slots(eng, oracle):
    """G = 20, S = 16 of the other fused routes' wide case: k_transit_grad's LDS [G + NP1][64] with 17 slots, NVMR = 18, a
    permuted gas map"""
    got = _check_case(eng, oracle, _wide_case())
    assert np.all(np.abs(got[2]).max(axis=(0, 2)) > 0)


@pytest.mark.parametrize("G,S", [(32, 3), (27, 5), (20, 31), (32, 31)])
def test_transit_at_the_size_limits(eng, oracle, G, S):
    """The (G, S) of the other fused routes' size cases (SIZE_CASES of test_limb_gpu.py).  This route has no chunk rule:
    k_transit_grad holds [G + NP1][64] doubles, 32 KiB at G = 32, S = 31, and reads gas 30 and the temperature from bits 30 and
    31 of the mask.  Same references and bounds as every case of this file."""
    from test_limb_gpu import assert_size_case
    assert_size_case(G, S)
    assert (G + S + 1) * 512 <= 64 * 1024
    got = _check_case(eng, oracle, _wide_case(G, S))
    assert np.all(np.abs(got[2]).max(axis=(0, 2)) > 0)


def test_transit_on_lbl_table(eng, oracle):
    """G = 1 on a line-by-line table, L = 5"""
    _check_case(eng, oracle, _case(130, L=5, lbl=True))


def test_transit_without_continuum_gradients(eng, oracle):
    got = _check_case(eng, oracle, _case(130), dcont=None)
    free = [k for k in range(NPAR) if k not in set(IGAS_MAP) | {NVMR}]
    assert np.all(got[2][:, free, :] == 0.0)


def test_transit_with_one_gas_masked(eng, oracle):
    eng.set_gradient_gases([0, 2], temperature=True)
    try:
        _check_case(eng, oracle, _case(130), gases={0, 2})
    finally:
        eng.set_gradient_gases(None)


def test_transit_with_a_pending_shared_gas_gradient(eng, oracle):
    c = _case(130)
    with_term = _check_case(eng, oracle, c, every_gas=True)
    without = _fused(eng, c)                             # consumed: the next call is without it
    assert not np.array_equal(with_term[2][:, :NVMR], without[2][:, :NVMR])
    assert np.array_equal(with_term[2][:, NVMR:], without[2][:, NVMR:]) and np.array_equal(with_term[0], without[0])


def test_transit_chain_to_the_state_vector_on_the_device(eng, oracle):
    """map2pro(None) / map2xvec(None) continue from the dAREA the fused call left on the device: the same as the host maps of
    the returned dAREA, within the map tests' 1e-13 of the slot's largest element."""
    c = _case(130)
    _upload(eng, c)
    W, L = c["W"], c["L"]
    rng = np.random.default_rng(3)
    NPRO, NX = 17, 9
    DTE, DAM, DCO = (rng.uniform(0, 1, (L, NPRO)) for _ in range(3))
    xmap = rng.normal(size=(NX, NPAR, NPRO))
    host = _fused(eng, c)
    with pytest.raises(ValueError):
        eng.map2pro(None, W, NVMR, NDUST, NPRO, 1, np.array([L]), np.arange(L), DTE, DAM, DCO)       # nothing was left to chain
    dev = _fused(eng, c, gradients_on_device=True)
    assert dev[2] is None and np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])
    pro = eng.map2pro(None, W, NVMR, NDUST, NPRO, 1, np.array([L]), np.arange(L), DTE, DAM, DCO)
    assert eng.map2pro(None, W, NVMR, NDUST, NPRO, 1, np.array([L]), np.arange(L), DTE, DAM, DCO, to_host=False) is None
    xv = eng.map2xvec(None, W, NVMR, NDUST, NPRO, 1, NX, xmap)
    pro_o = oracle.map2pro(host[2][..., None], W, NVMR, NDUST, NPRO, 1, np.array([L]), np.arange(L)[:, None], DTE, DAM, DCO)
    xv_o = oracle.map2xvec(pro_o, W, NVMR, NDUST, NPRO, 1, NX, xmap)
    assert pro.shape == (W, NPAR, NPRO, 1) and xv.shape == (W, 1, NX)
    for par in range(NPAR):
        np.testing.assert_allclose(pro[:, par], pro_o[:, par], rtol=0, atol=1e-13 * np.max(np.abs(pro_o[:, par])))
    np.testing.assert_allclose(xv, xv_o, rtol=0, atol=1e-13 * np.max(np.abs(xv_o)))


def test_transit_golden_c1(eng, oracle, golden_dir):
    """The reference's nemesisPTfm(gradients=True) on the cut C1 case through the real engine: depth rtol 2e-7 (float32 table
    grids), every column of dSPECMOD within max(16 x the fixture's restatement error, 1e-10) of its largest element -- a bound
    that stays below the 1e-4 contract."""
    z = np.load(os.path.join(golden_dir, "transit_c1.npz"))
    eng.upload_ktable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"], z["DELG"])
    L = z["LAY_PRESS"].size
    nvmr, ndust, npro = int(z["NVMR"]), int(z["NDUST"]), int(z["NPRO"])
    npar = nvmr + 2 + ndust
    tan = tc.tangent_heights_km(z["BASEH"], z["NLAYIN"], z["LAYINC"])
    c = tc.path_weights(tan, float(z["RADIUS"]))
    amount = np.ascontiguousarray(z["LAY_AMOUNT"].T) * 1.0e-4
    AREA, TRANS, dAREA = eng.cirsradg_ck_transit(z["LAY_PRESS"], z["LAY_TEMP"], amount, z["TAUCONT"], z["dTAUCON"], nvmr, npar,
                                                 z["igas_map"], z["NLAYIN"], z["LAYINC"], z["SCALE"], c, gradients_on_device=True)
    assert dAREA is None
    spec, fac = tc.depth(AREA, float(z["RADIUS"]), tan[0], float(z["RSTAR_KM"]))
    W, NX = spec.size, z["xmap"].shape[0]
    eng.map2pro(None, W, nvmr, ndust, npro, 1, np.array([L]), np.arange(L), z["DTE"], z["DAM"], z["DCO"], INCPAR=list(z["incpar"]),
                to_host=False)
    dspec = eng.map2xvec(None, W, nvmr, ndust, npro, 1, NX, z["xmap"])[:, 0, :] * fac
    ref = z["dSPECMOD"][:, 0, :]
    scale = np.abs(ref).max(axis=0)
    err = np.abs(dspec - ref).max(axis=0) / scale
    bound = np.maximum(16.0 * z["restatement_err"], 1e-10)
    print("depth rel %.3e; worst column %.3e of its largest element (bound there %.3e); worst err / bound %.3e"
          % (np.max(np.abs(spec / z["SPECMOD"][:, 0] - 1.0)), err.max(), bound[np.argmax(err)], np.max(err / bound)))
    assert bound.max() <= 1e-4
    np.testing.assert_allclose(spec, z["SPECMOD"][:, 0], rtol=2e-7)
    assert np.all(err <= bound)


def test_transit_conditions(eng, oracle):
    """Equal inputs, equal bits; an un-collapsed call before and after a fused call returns equal bits (no scratch of the one is
    the other's); the scratch beyond the gas stage stays within (2 L G + P) Wpad doubles: no factor P LIMAX NPAR."""
    c = _case(130)
    _upload(eng, c)
    before = eng.cirsradg_ck_transmission(c["lp"], c["lt"], c["am"], c["cont"], c["dcont"], NVMR, NPAR, IGAS_MAP, c["NLAYIN"],
                                          c["LAYINC"], c["SCALE"])
    a = _fused(eng, c)
    scratch, ms_sens, ms_grad = eng.transit_last()
    b = _fused(eng, c)
    after = eng.cirsradg_ck_transmission(c["lp"], c["lt"], c["am"], c["cont"], c["dcont"], NVMR, NPAR, IGAS_MAP, c["NLAYIN"],
                                         c["LAYINC"], c["SCALE"])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    L, P, G, Wpad = c["L"], c["NLAYIN"].size, 10, 192
    print("scratch %d bytes (bound %d), k_transit_sens %.3f ms, k_transit_grad %.3f ms" % (scratch, (2 * L * G + P) * Wpad * 8, ms_sens, ms_grad))
    assert 0 < scratch <= (2 * L * G + P) * Wpad * 8
    assert ms_sens > 0 and ms_grad > 0


def test_transit_layer_cap(eng, oracle):
    """L = 320 (the whole 160 KiB tile) runs and agrees with the un-collapsed route; L = 321 is NotImplementedError; paths that
    leave the layers or the LAYINC rows are ValueError."""
    c = _case(64, L=CAP, P=3)
    _upload(eng, c)
    got = _fused(eng, c)
    _compare("L = 320, same engine, un-collapsed", got, _uncollapsed_on_engine(eng, c, np.array(c["dcont"])), c["weight"])
    assert got[1].min() > 1e-200
    big = _case(64, L=CAP + 1, P=3)
    with pytest.raises(NotImplementedError):
        _fused(eng, big)
    small = _case(64)
    args = [small["lp"], small["lt"], small["am"], small["cont"], None, NVMR, NPAR, IGAS_MAP]
    bad = np.array(small["LAYINC"]); bad[1, 0] = small["L"]
    with pytest.raises(ValueError):
        eng.cirsradg_ck_transit(*args, small["NLAYIN"], bad, small["SCALE"], small["weight"])
    with pytest.raises(ValueError):
        eng.cirsradg_ck_transit(*args, small["NLAYIN"] + 1, small["LAYINC"], small["SCALE"], small["weight"])
    pads = np.array(small["LAYINC"]); pads[-1, 5] = 10 ** 6            # beyond NLAYIN[5]: padding, never read
    ok = eng.cirsradg_ck_transit(*args, small["NLAYIN"], pads, small["SCALE"], small["weight"])
    ref = eng.cirsradg_ck_transit(*args, small["NLAYIN"], small["LAYINC"], small["SCALE"], small["weight"])
    assert all(np.array_equal(x, y) for x, y in zip(ok, ref))
