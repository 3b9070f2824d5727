"""ansfm_cirsradg_ck_limb on the GPU (k_limb_planck, k_limb_sens, k_limb_grad): the thermal emission of the limb paths mixed to the
geometries of the measurement with their layer gradients, against the collapsed restatement (tests/limb_cases.py) on the CPU
oracle's opacities, against the un-collapsed route of the same engine (cirsradg_ck_thermal, then the restatement's mix), and
against the reference's nemesisLfmg in tests/golden/limb_c1.npz.

Tolerances are those the existing GPU tests hold this branch to: 1e-10 relative on a radiance (the thermal-gradient tests of
test_gpu_parity.py), 1e-10 of the parameter slab's largest element on a gradient (test_occultation_gpu.py; the thermal-gradient
tests ask 1e-9).  MOD[w, q] = xfac sum_p C[q, p] SPEC_p inherits 1e-10 max|xfac| sum_p |C[q, p]| max SPEC."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limb_cases as lc  # noqa: E402
import occultation_cases as oc  # noqa: E402
import transit_cases as tc  # noqa: E402
from test_transit_gpu import _case as _transit_case  # noqa: E402  (the synthetic generator: G = 10, S = 3, or G = 1 on an LBL table)

pytestmark = pytest.mark.gpu

NVMR, NDUST = 4, 1
NPAR = NVMR + 2 + NDUST
IGAS_MAP = np.array([2, 0, 3], dtype=np.int32)
CAP = 160                       # layers of the fused call (include/ansfm.h)


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


def _emtemp(c, rng):
    """EMTEMP of its own for every path entry: the layer's temperature moved by up to 3 K, so the two legs of a path differ"""
    LIMAX, P = c["LAYINC"].shape
    inside = np.arange(LIMAX)[:, None] < c["NLAYIN"][None, :]
    return np.where(inside, np.asarray(c["lt"])[c["LAYINC"]] + rng.uniform(-3.0, 3.0, (LIMAX, P)), 0.0)


@functools.lru_cache(maxsize=None)
def _case(W, L=12, lbl=False, kind="pairs"):
    """A case of test_transit_gpu._case with some of its limb paths (path p runs down to layer p and up again; SCALE is drawn
    per entry, EMTEMP too), and a mixing matrix.  pairs: Q = 3 geometries on 6 bracketing paths, two entries a row (L = 5: Q = 2
    on 4 paths).  shared: 5 paths, three geometries of which neighbours share a path (as calc_pathg_L leaves them after
    np.unique), the fifth path named by no geometry.  general: all L - 1 paths, C (5, L - 1) with dense rows, negative entries, an
    empty row and a row that names the last path only.  cap: 4 paths, Q = 2."""
    t = _transit_case(W, L, lbl)
    rng = np.random.default_rng(7 + W + 1000 * L)
    P0 = L - 1
    if kind == "pairs":
        keep = np.array([1, 2, 5, 6, 8, 9]) if L >= 12 else np.array([0, 1, 2, 3])
        Q = keep.size // 2
        C = np.zeros((Q, keep.size))
        for q in range(Q):
            f = rng.uniform(0.1, 0.9)
            C[q, 2 * q], C[q, 2 * q + 1] = 1.0 - f, f
    elif kind == "shared":
        keep = np.array([2, 3, 4, 5, 9])
        C = np.array([[0.3, 0.7, 0.0, 0.0, 0.0], [0.0, 0.55, 0.45, 0.0, 0.0], [0.0, 0.0, 0.2, 0.8, 0.0]])
    elif kind == "general":
        keep = np.arange(P0)
        C = np.zeros((5, P0))
        C[0] = rng.uniform(0.1, 1.0, P0)
        C[1] = rng.uniform(-1.0, 1.0, P0)
        C[3, P0 - 1] = 0.75                                   # row 2 stays empty
        C[4, [0, 3, 4]] = [-0.5, 2.0, 0.25]
    elif kind == "many":
        keep, C = np.arange(P0), many_geometries(P0, rng)
    else:                                                     # cap
        keep = np.linspace(0, L - 2, 4).astype(int)
        C = np.array([[0.3, 0.7, 0.0, 0.0], [0.0, 0.0, 0.6, 0.4]])
    c = {k: v for k, v in t.items() if k not in ("NLAYIN", "LAYINC", "SCALE", "weight")}
    c["NLAYIN"] = np.ascontiguousarray(t["NLAYIN"][keep])
    c["LAYINC"] = np.ascontiguousarray(t["LAYINC"][:, keep])
    c["SCALE"] = np.ascontiguousarray(t["SCALE"][:, keep])
    c["EMTEMP"] = _emtemp(c, rng)
    c["C"] = C
    c["xfac"] = rng.uniform(0.5, 2.0, W) * 1.0e3
    c["G"] = 1 if lbl else 10
    return _freeze(c)


def many_geometries(P0, rng):
    """C (9, P0), P0 >= 9: geometry q mixes the successive tangent paths q and q + 1 (paths 4 and 5 go to geometry 5, and so on
    past the gap) and row 4 is empty.  Path p turns in layer p, so the geometries with an entry in a layer fall from 8 in the top
    layers to 1 in layer 0: more than the kMixWaves = 4 waves of a contraction block, which then serve two geometries each, and
    behind the empty row the geometry's index and its turn among the waves differ."""
    C = np.zeros((9, P0))
    for q in (0, 1, 2, 3, 5, 6, 7, 8):
        f = rng.uniform(0.1, 0.9)
        j = q if q < 4 else q - 1
        C[q, j], C[q, j + 1] = 1.0 - f, f
    return C


# --- the slot chunk of the contraction, restated (slab_chunk of csrc/ansfm_pathmix_kernels.hip.h) ---------------------------------
MIX_WAVES, MIX_LDS_TWO_BLOCKS, MIX_LDS_ONE_BLOCK = 4, 80 * 1024, 160 * 1024


def slab_chunk(G, NP1):
    """(slots a chunk, LDS bytes of a block): a row is one g-ordinate's 512 B per slot, the waves' columns take MIX_WAVES rows of G"""
    row = G * 512
    budget = MIX_LDS_TWO_BLOCKS if MIX_LDS_TWO_BLOCKS >= (MIX_WAVES + 1) * row else MIX_LDS_ONE_BLOCK
    chunks = -(-NP1 // min((budget - MIX_WAVES * row) // row, NP1))
    return -(-NP1 // chunks), (MIX_WAVES + -(-NP1 // chunks)) * row


# (G, S) -> (slots a chunk, chunks, LDS bytes) the size cases of the four fused routes are meant to reach
SIZE_CASES = {(32, 3): (1, 4, 80 * 1024),        # no slot to spare: cols + row is the two-block budget exactly
              (27, 5): (1, 6, 67.5 * 1024),      # one slot a chunk with 12.5 KiB left over
              (20, 31): (4, 8, 80 * 1024),       # 32 slots in 8 chunks of 4
              (32, 31): (1, 32, 80 * 1024)}      # 32 chunks of 1


def assert_size_case(G, S):
    sc, lds = slab_chunk(G, S + 1)
    assert (sc, -(-(S + 1) // sc), lds) == SIZE_CASES[(G, S)]
    return sc, lds


@functools.lru_cache(maxsize=None)
def _wide_case(G=20, S=16, kind="two", seed=92, emtemp=True):
    """L = 4, W = 64, NVMR = S + 2.  G = 20, S = 16: 17 slots of 10 KiB beside 40 KiB of columns, more than one LDS stage holds.
    Any other (G, S) is a size case (SIZE_CASES): its amounts are scaled by one factor so that the gas opacity along a path at
    g = 3 G // 4, median over wavenumbers and paths, is 1 -- unscaled, 31 gases leave exp(-tau_path) = 0 at the upper g-ordinates,
    and their weights and register slots would test nothing.  kind "two": Q = 2 geometries on the 3 limb paths.  seed and emtemp
    are for the occultation and transit files, which draw the same arrays from a seed of their own without EMTEMP."""
    from archnemesis_dist_amd import synthetic as syn
    assert kind == "two"
    W, L = 64, 4
    default = (G, S) == (20, 16)
    rng = np.random.default_rng(seed if default else [seed, G, S])
    c = dict(W=W, L=L, S=S, lbl=False, G=G, tag=("wide", seed))
    c["PRESS"], c["TEMP"], c["K"] = syn.synth_ktable(W, G, 6, 5, S, seed=23)
    c["delg"] = syn.gauss_legendre_01(G)[1]
    c["WAVE"] = 900.0 + 0.7 * np.arange(W)
    c["lp"] = np.logspace(4.5, 2.5, L); c["lt"] = np.linspace(200, 160, L)
    c["am"] = 10.0 ** rng.uniform(17, 18.5, (S, L)) * (c["lp"][None, :] / c["lp"][:1])
    c["cont"] = 10.0 ** rng.uniform(-4, -1, (W, L))
    c["NVMR"] = S + 2
    c["NPAR"] = S + 2 + 2 + NDUST
    c["igas_map"] = rng.permutation(S + 2)[:S].astype(np.int32)
    c["dcont"] = 10.0 ** rng.uniform(-24, -22, (W, c["NPAR"], L))
    c["NLAYIN"], c["LAYINC"], c["SCALE"] = tc.limb_paths(L, rng)
    if emtemp:
        c["EMTEMP"] = _emtemp(c, rng)
    c["C"] = np.array([[0.4, 0.6, 0.0], [0.0, 0.2, 0.8]])
    c["xfac"] = rng.uniform(0.5, 2.0, W)
    if not default:
        from oracle import oracle as orc
        orc.build()
        k = orc.calc_k(c["K"], c["PRESS"], c["TEMP"], c["lp"] / 101325.0, c["lt"])
        along = np.einsum("wl,lp->wp", orc.k_overlap(c["delg"], k, c["am"])[:, 3 * G // 4, :],
                          tc.path_matrix(L, c["NLAYIN"], c["LAYINC"], c["SCALE"]))
        c["am"] = c["am"] / np.median(along)
    return _freeze(c)


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


def _fused(eng, c, dcont="dcont", xfac=True, ispace=0, **kw):
    nvmr, npar, ig = _dims(c)
    return eng.cirsradg_ck_limb(ispace, c["lp"], c["lt"], c["am"], c["cont"], None if dcont is None else c[dcont], nvmr, npar, ig,
                                c["NLAYIN"], c["LAYINC"], c["SCALE"], c["EMTEMP"], c["C"], xfac=c["xfac"] if xfac else None, **kw)


def _thermal(eng, c, dcont, xfac=True, ispace=0):
    nvmr, npar, ig = _dims(c)
    return eng.cirsradg_ck_thermal(ispace, c["lp"], c["lt"], c["am"], c["cont"], dcont, nvmr, npar, ig, c["NLAYIN"], c["LAYINC"],
                                   c["SCALE"], c["EMTEMP"], -1.0, xfac=c["xfac"] if xfac else None)


def _uncollapsed_on_engine(eng, c, dcont, xfac=True, ispace=0):
    spec, dspec, _ = _thermal(eng, c, dcont, xfac, ispace)
    MOD, dMOD = oc.mod_from_paths(spec, dspec, c["C"], c["NLAYIN"], c["LAYINC"], c["L"])
    return MOD, spec / (c["xfac"][:, None] if xfac else 1.0), dMOD


def _compare(what, got, ref, C, xfmax):
    (MOD, SPEC, dMOD), (rM, rS, rdM) = got, ref
    scale = np.max(np.abs(rdM), axis=(0, 2, 3), keepdims=True)
    err = np.max(np.abs(dMOD - rdM) / np.where(scale > 0, scale, 1.0), axis=(0, 2, 3))
    atol = 1e-10 * xfmax * np.abs(C).sum(axis=1) * rS.max()
    print("%s: SPEC rel %.3e, MOD / its bound %.3e, dMOD by parameter %s" % (
        what, np.max(np.abs(SPEC - rS) / rS), np.max(np.abs(MOD - rM) / np.where(atol > 0, atol, 1.0)[None, :]),
        np.array2string(err, precision=2)))
    np.testing.assert_allclose(SPEC, rS, rtol=1e-10)
    assert np.all(np.abs(MOD - rM) <= atol[None, :])
    assert err.max() < 1e-10
    assert np.all(dMOD[:, scale.reshape(-1) == 0] == 0.0)


def _check_case(eng, oracle, c, dcont="dcont", xfac=True, ispace=0, gases=None, temperature=True, every_gas=False):
    nvmr, npar, ig = _dims(c)
    _upload(eng, c)
    got = _fused(eng, c, dcont, xfac, ispace, dtau_every_gas=c["dray"] if every_gas else None)
    Q, P = c["C"].shape
    assert got[0].shape == (c["W"], Q) and got[1].shape == (c["W"], P) and got[2].shape == (c["W"], npar, c["L"], Q)
    tautot, dk = _opacities(oracle, c)
    dtau = tc.dtautot(dk, ig, nvmr, npar, None if dcont is None else c[dcont], c["dray"] if every_gas else None,
                      gases=gases, temperature=temperature)
    xf = c["xfac"] if xfac else None
    ref = lc.collapsed(tautot, np.asarray(c["delg"], dtype=np.float64), c["NLAYIN"], c["LAYINC"], c["SCALE"], c["EMTEMP"], c["C"],
                       ispace, c["WAVE"], nvmr, dtau, xf)
    assert np.abs(ref[2]).max() > 0 and ref[1].min() > 1e-300
    xfmax = float(np.abs(c["xfac"]).max()) if xfac else 1.0
    _compare("oracle, collapsed", got, ref, c["C"], xfmax)
    dc = None if dcont is None else np.array(c[dcont])
    if every_gas:                                        # the un-collapsed call takes the shared term inside dtaucon
        dc = np.zeros((c["W"], npar, c["L"])) if dc is None else dc
        dc[:, :nvmr, :] += c["dray"][:, None, :]
    _compare("same engine, un-collapsed", got, _uncollapsed_on_engine(eng, c, dc, xfac, ispace), c["C"], xfmax)
    # a (layer, geometry) pair no path of the geometry crosses is exactly zero
    Sm = tc.path_matrix(c["L"], c["NLAYIN"], c["LAYINC"], np.ones_like(c["SCALE"]))
    touched = (Sm != 0.0).astype(float) @ (c["C"] != 0.0).T.astype(float) > 0          # (L, Q)
    assert np.all(got[2][:, :, ~touched] == 0.0)
    return got


@pytest.mark.parametrize("xfac,ispace", [(True, 0), (False, 0), (True, 1)])
def test_limb_vs_oracle_and_vs_uncollapsed_route(eng, oracle, xfac, ispace):
    """W = 130: three wavenumber tiles, the last with two live lanes; G = 10, S = 3, L = 12, Q = 3 geometries on the 6 limb paths
    that bracket them (two entries a row), the legs of every path with their own SCALE and EMTEMP, NVMR = 4, NDUST = 1,
    igas_map [2, 0, 3], random dTAUCON; with and without xfac; on a wavenumber (ISPACE 0) and a wavelength (ISPACE 1) axis."""
    c = _case(130)
    assert c["C"].shape == (3, 6) and np.all((c["C"] != 0).sum(axis=1) == 2)
    n0 = int(c["NLAYIN"][0])
    assert not np.array_equal(c["EMTEMP"][:n0 // 2, 0], c["EMTEMP"][n0 - 1:n0 // 2 - 1:-1, 0])
    assert not np.array_equal(c["SCALE"][:n0 // 2, 0], c["SCALE"][n0 - 1:n0 // 2 - 1:-1, 0])
    _check_case(eng, oracle, c, xfac=xfac, ispace=ispace)


@pytest.mark.parametrize("W", [64, 1])
def test_limb_whole_tile_and_single_wavenumber(eng, oracle, W):
    _check_case(eng, oracle, _case(W))


def test_limb_adjacent_geometries_share_a_path(eng, oracle):
    """Three geometries on four paths, neighbours sharing one (ITANHE of calc_pathg_L is np.unique'd); a fifth path that no
    geometry names still gets its SPEC"""
    c = _case(130, kind="shared")
    got = _check_case(eng, oracle, c)
    assert got[1][:, 4].min() > 0


def test_limb_general_mixing_matrix(eng, oracle):
    """C (5, 11): a dense row, a row with negative entries, an empty row (MOD and dMOD exactly 0), a row that names the last
    path only, a row of three"""
    c = _case(130, kind="general")
    got = _check_case(eng, oracle, c)
    assert np.all(got[0][:, 2] == 0.0) and np.all(got[2][..., 2] == 0.0)
    assert np.array_equal(got[0][:, 3], c["xfac"] * (0.75 * got[1][:, -1]))
    # the same matrix as compressed rows
    nz = c["C"] != 0
    triple = (np.concatenate([[0], np.cumsum(nz.sum(axis=1))]), np.nonzero(nz)[1], c["C"][nz])
    again = eng.cirsradg_ck_limb(0, c["lp"], c["lt"], c["am"], c["cont"], c["dcont"], NVMR, NPAR, IGAS_MAP, c["NLAYIN"], c["LAYINC"],
                                 c["SCALE"], c["EMTEMP"], triple, xfac=c["xfac"])
    assert all(np.array_equal(x, y) for x, y in zip(got, again))


def test_limb_five_layers_and_lbl_table(eng, oracle):
    """L = 5 on the k-table, and G = 1 on a line-by-line table"""
    _check_case(eng, oracle, _case(130, L=5))
    _check_case(eng, oracle, _case(130, L=5, lbl=True))


def test_limb_without_continuum_gradients(eng, oracle):
    got = _check_case(eng, oracle, _case(130), dcont=None)
    free = [k for k in range(NPAR) if k not in set(IGAS_MAP) | {NVMR}]
    assert np.all(got[2][:, free] == 0.0)


def test_limb_with_one_gas_masked(eng, oracle):
    eng.set_gradient_gases([0, 2], temperature=True)
    try:
        _check_case(eng, oracle, _case(130), gases={0, 2})
    finally:
        eng.set_gradient_gases(None)


def test_limb_with_a_pending_shared_gas_gradient(eng, oracle):
    c = _case(130)
    with_term = _check_case(eng, oracle, c, every_gas=True)
    without = _fused(eng, c)                             # consumed: the next call is without it
    assert not np.array_equal(with_term[2][:, :NVMR], without[2][:, :NVMR])
    assert np.array_equal(with_term[2][:, NVMR:], without[2][:, NVMR:]) and np.array_equal(with_term[0], without[0])


def test_limb_slab_beyond_one_lds_stage(eng, oracle):
    """G = 20, S = 16: the 17 slots of the layer's slab go through LDS in chunks; every parameter, whichever chunk its slot lies
    in, agrees, and the parameters without a slot come with the first chunk"""
    c = _wide_case()
    got = _check_case(eng, oracle, c)
    assert np.all(np.abs(got[2]).max(axis=(0, 2, 3)) > 0)


@pytest.mark.parametrize("G,S", sorted(SIZE_CASES))
def test_limb_at_the_size_limits(eng, oracle, G, S):
    """The chunk rule at its edges (SIZE_CASES; the restated slab_chunk keeps each case on its edge): 32 g-ordinates, where the
    waves' columns and one slot are the two-block budget exactly; 31 gases, the 32 slots in 8 chunks of 4 and in 32 chunks of 1,
    gas 30 and the temperature on bits 30 and 31 of the mask.  Same references and bounds as every case of this file."""
    assert_size_case(G, S)
    c = _wide_case(G, S)
    got = _check_case(eng, oracle, c)
    assert np.all(np.abs(got[2]).max(axis=(0, 2, 3)) > 0)


def test_limb_more_geometries_than_waves(eng, oracle):
    """Q = 9 on the 11 tangent paths (many_geometries): in the top layers 8 geometries have an entry and every wave of the block
    serves two, filling its LDS columns again for the second; row 4 is empty."""
    c = _case(130, kind="many")
    Sm = tc.path_matrix(c["L"], c["NLAYIN"], c["LAYINC"], c["SCALE"])
    entries = ((Sm != 0.0).astype(float) @ (c["C"] != 0.0).T.astype(float) > 0).sum(axis=1)          # geometries by layer
    assert c["C"].shape == (9, 11) and entries.max() >= 6 and entries.min() == 1 and not np.any(c["C"][4])
    got = _check_case(eng, oracle, c)
    assert np.all(got[0][:, 4] == 0.0) and np.all(got[2][..., 4] == 0.0)


def test_limb_chain_to_the_state_vector_on_the_device(eng, oracle):
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


def test_last_of_each_fused_route_keeps_its_own_call():
    """transit, occultation and limb keep separate records on one engine: after one call of each (W = 130, L = 12, the `pairs`
    case of each file), every *_last returns the scratch bytes its call reported on an engine of its own, and times >= 0; on the
    engine that ran the limb call only, the other two still have nothing recorded."""
    import archnemesis_dist_amd as pkg
    import test_occultation_gpu as tog
    import test_transit_gpu as ttg
    routes = [("transit", _transit_case(130), ttg._fused), ("occultation", tog._case(130), tog._fused), ("limb", _case(130), _fused)]
    alone = {}
    for name, c, call in routes:
        e = pkg.AnsfmEngine(0)
        try:
            _upload(e, c)
            call(e, c)
            alone[name] = getattr(e, name + "_last")()[0]
            if name == "limb":
                for other in (e.occultation_last, e.transit_last):
                    with pytest.raises(ValueError, match="call recorded yet"):
                        other()
        finally:
            e.close()
    assert len(set(alone.values())) == 3 and min(alone.values()) > 0
    e = pkg.AnsfmEngine(0)
    try:
        for name, c, call in routes:
            _upload(e, c)
            call(e, c)
        for name, c, call in routes:
            scratch, ms_a, ms_b = getattr(e, name + "_last")()
            assert scratch == alone[name], name
            assert ms_a >= 0.0 and ms_b >= 0.0, name
    finally:
        e.close()


def test_limb_conditions(eng, oracle):
    """Equal inputs, equal bits; an un-collapsed call before and after a fused call returns equal bits (no scratch of the one is
    the other's); the scratch beyond the gas stage and dMOD is exactly what include/ansfm.h states.  That formula stays below the
    8 W NPAR LIMAX P bytes of the array the call replaces at the shape the issue names (W 1024, G 20, L 100, P 20, LIMAX 200,
    NPAR 10, Q 10: 202 MB against 328 MB, arithmetic asserted here) but not at every shape: the scratch pads W to 64 lanes and
    does not shrink with NPAR, so at this test's W = 130 (Wpad 192), NPAR = 7 and one EMTEMP value per path entry it is 1.13 MB
    against 1.05 MB, and at W = 1 sixty times the array.  include/ansfm.h says so; the entry does not refuse such shapes."""
    c = _case(130)
    _upload(eng, c)
    unc = lambda: _thermal(eng, c, c["dcont"])
    before = unc()
    a = _fused(eng, c)
    scratch, ms_sens, ms_grad = eng.limb_last()
    b = _fused(eng, c)
    after = unc()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    (Q, P), G, Wpad, W, L = c["C"].shape, 10, 192, 130, c["L"]
    NT = np.unique(c["EMTEMP"][np.arange(c["LAYINC"].shape[0])[:, None] < c["NLAYIN"][None, :]]).size
    stated = 8 * Wpad * (Q * L * (G + 4) + P * G + 2 * NT) + 8 * W * (Q + P)
    replaced = 8 * W * NPAR * c["LAYINC"].shape[0] * P
    print("scratch %d bytes (replaced array %d; dMOD %d), k_limb_planck + k_limb_sens %.3f ms, k_limb_grad %.3f ms"
          % (scratch, replaced, a[2].nbytes, ms_sens, ms_grad))
    assert scratch == stated
    at_issue_shape = 8 * 1024 * (10 * 100 * (20 + 4) + 20 * 20 + 2 * 100) + 8 * 1024 * (10 + 20)
    assert at_issue_shape == 201768960 and at_issue_shape < 8 * 1024 * 10 * 200 * 20
    assert ms_sens > 0 and ms_grad > 0


def test_limb_layer_cap_ground_path_and_invalid_arguments(eng, oracle):
    """L = 160 (the whole 160 KiB of LDS in k_limb_sens) with P = 4, Q = 2 runs and agrees with the un-collapsed route; L = 161 is
    NotImplementedError, and so is a path that ends at the lower boundary; paths that leave the layers or the LAYINC rows and mix
    entries that leave the paths are ValueError; padding beyond NLAYIN is never read."""
    c = _case(64, L=CAP, kind="cap")
    _upload(eng, c)
    got = _fused(eng, c)
    _compare("L = 160, same engine, un-collapsed", got, _uncollapsed_on_engine(eng, c, np.array(c["dcont"])), c["C"],
             float(c["xfac"].max()))
    with pytest.raises(NotImplementedError):
        _fused(eng, _case(64, L=CAP + 1, kind="cap"))
    small = _case(64)
    Q, P = small["C"].shape
    args = [0, small["lp"], small["lt"], small["am"], small["cont"], None, NVMR, NPAR, IGAS_MAP]
    call = lambda nlayin, layinc, mix: eng.cirsradg_ck_limb(*args, nlayin, layinc, small["SCALE"], small["EMTEMP"], mix)
    _upload(eng, small)
    ground = np.array(small["LAYINC"]); ground[:small["L"], 0] = np.arange(small["L"] - 1, -1, -1)      # top to bottom, and no way up
    nground = np.array(small["NLAYIN"]); nground[0] = small["L"]
    with pytest.raises(NotImplementedError):
        call(nground, ground, small["C"])
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
    with pytest.raises(ValueError):
        call(small["NLAYIN"], small["LAYINC"], (np.array([1, 2, 3, 3]), np.array([0, 1, 2]), np.ones(3)))      # rows that start at 1
    pads = np.array(small["LAYINC"]); pads[-1, 5] = 10 ** 6            # beyond NLAYIN[5]: padding, never read
    ok = call(small["NLAYIN"], pads, small["C"])
    ref = call(small["NLAYIN"], small["LAYINC"], small["C"])
    assert all(np.array_equal(x, y) for x, y in zip(ok, ref))


def test_limb_golden_c1(eng, oracle, golden_dir):
    """The reference's nemesisLfmg on the cut C1 case (three tangent heights on six bracketing paths) through the real engine
    and the device chain: SPECMOD rtol 2e-7 (float32 table grids), every non-zero column of dSPECMOD within
    max(16 x the fixture's restatement error, 1e-10) of its largest element plus the derived allowance for the cancellation in
    T_{j-1} - T_j that stands at the bound below (nothing for most columns, up to 3.8e-5 for the topmost temperature level) -- and
    the columns the reference leaves zero exactly zero."""
    from archnemesis_dist_amd import limb
    z = np.load(os.path.join(golden_dir, "limb_c1.npz"))
    eng.upload_ktable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"], z["DELG"])
    L = z["LAY_PRESS"].size
    nvmr, ndust, npro = int(z["NVMR"]), int(z["NDUST"]), int(z["NPRO"])
    npar = nvmr + 2 + ndust
    tan = limb.tangent_heights_km(z["BASEH"], z["NLAYIN"], z["LAYINC"])
    C = limb.tangent_mix(tan, z["TANHE"])
    Q = C.shape[0]
    amount = np.ascontiguousarray(z["LAY_AMOUNT"].T) * 1.0e-4
    MOD, SPEC, dMOD = eng.cirsradg_ck_limb(int(z["ISPACE"]), z["LAY_PRESS"], z["LAY_TEMP"], amount, z["TAUCONT"], z["dTAUCON"], nvmr,
                                           npar, z["igas_map"], z["NLAYIN"], z["LAYINC"], z["SCALE"], z["EMTEMP"], C, xfac=z["XFAC"],
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
    # 1e-10 of a column's largest element (test_occultation_gpu.py) plus what the rounding of d_j = T_{j-1} - T_j allows: the device's
    # exp and NumPy's may differ by an ulp, and with the product and the subtraction d_j carries up to 4 x 2^-53 T_{j-1} whatever
    # tau_j is, which in the thin top layers (tau ~ 1e-9) is 1e-7 of d_j itself.  lc.cancellation_terms carries that through the
    # linear algebra with absolute values.  On this fixture the term stays below 1e-10 for the first 67 columns (the gases, the
    # continuum and the lower temperature levels) and reaches 3.8e-5 for the topmost temperature level, below the 1e-4 contract.
    cancel = 4.0 * 2.0 ** -53 * lc.golden_cancellation_by_column(z, oracle)
    bound = np.maximum(16.0 * z["restatement_err"], 1e-10) + cancel
    assert np.count_nonzero(cancel[nonzero] < 1e-10) >= 45 and cancel.max() < 5e-5
    print("columns by err / bound:", np.array2string((err / bound)[nonzero], precision=2))
    print("columns by err:", np.array2string(err[nonzero], precision=2))
    print("SPECMOD rel %.3e; worst column %.3e of its largest element (bound there %.3e); worst err / bound %.3e"
          % (np.max(np.abs(MOD / z["SPECMOD"] - 1.0)), err[nonzero].max(), bound[np.argmax(np.where(nonzero, err, 0.0))],
             np.max((err / bound)[nonzero])))
    assert bound.shape == (NX,) and bound.max() <= 1e-4
    np.testing.assert_allclose(MOD, z["SPECMOD"], rtol=2e-7)
    assert np.all(err[nonzero] <= bound[nonzero])
    assert np.all(dspec[:, :, ~nonzero] == 0.0)
