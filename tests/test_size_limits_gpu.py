"""The RT and gradient kernels at the top of the supported sizes: 32 g-ordinates (ANSFM_MAX_NG), 31 spectroscopic gases with
gradients (NP1 = S + 1 <= 32; bit 31 of the gas mask is the temperature slot), and just beyond them, where the entries refuse.

  k_thermal_rt      8 g-groups with kGPer = 4 register slots each; slot 3 serves g >= 24.  The builds <false>, <true>, and the
                    pair <false, 1> / <true, 2> of a de-duplicated batch are separate compilations.
  k_thermal_rtg     launch_rtg takes GY = 16 g-groups for NP1 <= 14, 8 for NP1 <= 30, 4 for NP1 = 31, 32 -- kMaxG / GY = 2, 4, 8
                    register slots a thread; the GY = 4 build takes 4 (NP1 + 2) 512 B > 64 KiB of dynamic LDS.
  fill_slot_of_param, the gas mask: bits 30 and 31, two gases on one parameter column, S = 32.

Every GPU case is compared with the CPU oracle at the bounds the suite holds these entries to (test_gpu_parity.py): 1e-10 relative
on spectra and dTSURF, 1e-9 of the parameter slab's largest element on the gradient of the thermal RT, 1e-11 / 1e-10 on the
transmission and its gradient.  The fused routes' cases at the same limits are in test_transit_gpu.py, test_occultation_gpu.py,
test_limb_gpu.py and test_disc_gpu.py.

The tests of this file without the gpu mark run on the CPU oracle alone.  They are conditions on the inputs of the GPU cases here
and in the four files: that the expected result of every case moves by at least 1e-4 of its scale -- a million times the
tolerance -- when the weights of g >= 24 are zeroed, when the last gas slot of dk is zeroed, and when geometries 4 and 8 change
places; and that the restated slab_chunk puts every size case on the edge it is meant to reach."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import disc_cases as dc  # noqa: E402
import limb_cases as lc  # noqa: E402
import occultation_cases as oc  # noqa: E402
import transit_cases as tc  # noqa: E402
import test_disc_gpu as tdg  # noqa: E402
import test_limb_gpu as tlg  # noqa: E402
import test_occultation_gpu as tog  # noqa: E402
import test_transit_gpu as ttg  # noqa: E402

W, L, NDUST, TSURF = 70, 8, 1, 280.0            # W: two wavenumber tiles, six live lanes in the last
GRADIENT_CASES = [(32, 13), (32, 14), (32, 29), (20, 30), (32, 31), (3, 30), (25, 3)]
FORWARD_CASES = [(25, 5), (32, 5)]
MOVE = 1e-4                                     # of the quantity's scale: a million times the tolerance of 1e-10


def launch_rtg_groups(NP1):
    """GY of launch_rtg (csrc/ansfm_rt.hip): the largest of 16, 8, 4 whose reduction buffer [NP1 + 2][GY][64] stays within 128 KiB"""
    return next((gy for gy in (16, 8) if gy * (NP1 + 2) * 512 <= 128 * 1024), 4)


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


_CASES = {}


def _case(oracle, G, S, igas_map=None):
    """The shared builder: a nadir path at 25 degrees through L = 8 layers of synth_atmosphere, a synthetic table, a random
    continuum and dTAUCON, NVMR = S + 2, NDUST = 1, igas_map a random selection of the NVMR columns (or the one given), a surface
    at 280 K with a rising emissivity.  The amounts are multiplied by one factor so that the oracle's column optical depth at
    g = G // 2, median over wavenumbers, is 1: unscaled the synthetic atmosphere is optically thick by orders of magnitude at
    S = 31 and the lower layers would test nothing.  Then the column is thin at g = 0 and thick at g = G - 1 (asserted)."""
    key = (G, S, None if igas_map is None else tuple(igas_map))
    if key in _CASES:
        return _CASES[key]
    from archnemesis_dist_amd import synthetic as syn
    rng = np.random.default_rng([17, G, S])
    c = dict(G=G, S=S)
    c["PRESS"], c["TEMP"], c["K"] = syn.synth_ktable(W, G, 6, 5, S, seed=300 + 40 * G + S)
    c["delg"] = syn.gauss_legendre_01(G)[1]
    c["WAVE"] = 400.0 + 0.5 * np.arange(W)
    atm = syn.synth_atmosphere(L, S, seed=6)
    c["lp"], c["lt"], am = atm["lay_press_pa"][0], atm["lay_temp"][0], atm["amount"][0]
    c["NLAYIN"], c["LAYINC"], c["SCALE"] = syn.nadir_path(L, 25.0)
    c["EMTEMP"] = c["lt"][c["LAYINC"][:, 0]][:, None]
    c["cont"] = 10.0 ** rng.uniform(-4, -2, (W, L))
    c["NVMR"] = S + 2
    c["NPAR"] = c["NVMR"] + 2 + NDUST
    c["igas_map"] = (rng.permutation(c["NVMR"])[:S] if igas_map is None else np.array(igas_map)).astype(np.int32)
    c["dcont"] = c["cont"][:, None, :] * rng.uniform(0.0, 1e-22, (W, c["NPAR"], L))
    c["emis"] = np.linspace(0.8, 1.0, W)
    c["xfac"] = np.linspace(1.0, 1.5, W)
    column = lambda amount: _forward_oracle(oracle, c, amount=amount, taugas=True)[1].sum(axis=2)          # (W, G)
    c["am"] = am / np.median(column(am)[:, G // 2])
    c["spec"], tg = _forward_oracle(oracle, c, taugas=True)
    c["column"] = np.median(tg.sum(axis=2), axis=0)                                                        # (G,)
    assert abs(c["column"][G // 2] - 1.0) < 1e-6 and c["column"][0] < 0.3 and c["column"][G - 1] > 3.0, c["column"]
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    _CASES[key] = c
    return c


def _forward_oracle(oracle, c, amount=None, taugas=False, lt=None, cont=None, tsurf=TSURF):
    lt = c["lt"] if lt is None else lt
    return oracle.cirsrad_ck_thermal(0, c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"], c["lp"], lt, c["am"] if amount is None else amount,
                                     c["cont"] if cont is None else cont, c["NLAYIN"], c["LAYINC"], c["SCALE"], lt[c["LAYINC"][:, 0]][:, None],
                                     tsurf, EMISSIVITY=c["emis"], xfac=c["xfac"], return_taugas=taugas)


def _gradient_oracle(oracle, c, amount=None):
    """SPECOUT (W, 1), dSPECOUT (W, NPAR, L, 1), dTSURF (W, 1) of the case by the oracle's CIRSrad; the case's own once"""
    if amount is None and "grad" in c:
        return c["grad"]
    ref = oracle.cirsradg_ck_thermal(0, c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"], c["lp"], c["lt"], c["am"] if amount is None else amount,
                                     c["cont"], c["dcont"], c["NVMR"], c["NPAR"], c["igas_map"], c["NLAYIN"], c["LAYINC"], c["SCALE"],
                                     c["EMTEMP"], TSURF, EMISSIVITY=c["emis"], xfac=c["xfac"])
    if amount is None:
        for a in ref:
            a.flags.writeable = False
        # every gas column and the temperature column carry a gradient, and the surface is seen at every wavenumber
        assert np.all(np.abs(ref[1][:, list(c["igas_map"]) + [c["NVMR"]]]).max(axis=(0, 2, 3)) > 0) and np.all(ref[2] > 0)
        c["grad"] = ref
    return ref


def _merge(oracle, c):
    """tau (W, G, L) and dk (W, G, L, S + 1) of the case's gradient merge by the oracle, once"""
    if "merge" not in c:
        k, dkdT = oracle.calc_k(c["K"], c["PRESS"], c["TEMP"], c["lp"] / 101325.0, c["lt"], grad=True)
        c["merge"] = oracle.k_overlapg(c["delg"], k, dkdT, c["am"])
    return c["merge"]


def _restated(oracle, c, weights=None, dk=None, gases=None, temperature=True):
    """The oracle's CIRSrad(return_grad=True) put together from its parts -- calc_kg, k_overlapg, the assembly of dTAUTOT
    (transit_cases.dtautot), calc_thermal_emission_spectrumg on the path, the g-quadrature -- so that one part can be changed:
    the quadrature weights, dk, the gas selection.  -> SPECOUT (W, 1), dSPECOUT (W, NPAR, L, 1), dTSURF (W, 1)"""
    tau, dk0 = _merge(oracle, c)
    dtau = tc.dtautot(dk0 if dk is None else dk, c["igas_map"], c["NVMR"], c["NPAR"], c["dcont"], gases=gases, temperature=temperature)
    li, sc = c["LAYINC"][:, 0], c["SCALE"][:, 0]
    sg, dsg, dtsg = oracle.calc_thermal_emission_spectrumg(0, c["WAVE"], (tau + c["cont"][:, None, :])[:, :, li] * sc, dtau[:, :, :, li] * sc,
                                                           c["NVMR"], c["EMTEMP"][:, 0], c["lp"][li], TSURF, c["emis"])
    w, xf = np.asarray(c["delg"] if weights is None else weights, dtype=np.float64), c["xfac"]
    return ((sg @ w) * xf)[:, None], np.nan_to_num(np.einsum("wgkl,g->wkl", dsg, w) * xf[:, None, None])[..., None], ((dtsg @ w) * xf)[:, None]


def _slab_err(got, ref):
    """the largest error of dSPECOUT (W, NPAR, LIMAX, P) by parameter, in units of the parameter slab's largest element"""
    scale = np.abs(ref).max(axis=(0, 2, 3))
    assert np.all(got[:, scale == 0] == 0.0)
    return np.abs(got - ref).max(axis=(0, 2, 3)) / np.where(scale > 0, scale, 1.0)


def _moves(what, new, old, axes=None):
    """max |new - old| >= MOVE max |old|, over the whole array or for every index of the axes that are not reduced"""
    move, scale = np.abs(new - old).max(axis=axes), np.abs(old).max(axis=axes)
    assert np.all(scale > 0) and np.all(move >= MOVE * scale), (what, np.min(move / scale))
    return float(np.min(move / scale))


def _without_upper_g(c):
    w = np.array(c["delg"], dtype=np.float64)
    w[24:] = 0.0
    return w


def _without_last_gas(dk):
    out = np.array(dk)
    out[..., -2] = 0.0                           # slots 0 .. S - 1 are the gases, slot S the temperature
    return out


# ---- conditions on the inputs, on the CPU ------------------------------------------------------------------------------------------

def test_size_cases_sit_on_their_edges():
    """The restated slab_chunk (test_limb_gpu.py) gives every size case of the fused routes the chunk and the LDS bytes it is
    meant to reach; at G = 32 the columns and one slot are the two-block budget exactly, so one more g-ordinate would move to the
    one-block budget -- which no G <= ANSFM_MAX_NG = 32 reaches, because 5 G 512 <= 81 920."""
    for G, S in tlg.SIZE_CASES:
        tlg.assert_size_case(G, S)
    assert (tlg.MIX_WAVES + 1) * 32 * 512 == tlg.MIX_LDS_TWO_BLOCKS
    for G in range(1, 33):
        for NP1 in range(1, 33):
            sc, lds = tlg.slab_chunk(G, NP1)
            assert 1 <= sc <= NP1 and lds == (tlg.MIX_WAVES + sc) * G * 512 <= tlg.MIX_LDS_TWO_BLOCKS
    assert tlg.slab_chunk(33, 4) == (4, 8 * 33 * 512)                   # what the other branch would do
    assert [launch_rtg_groups(n) for n in (4, 14, 15, 30, 31, 32)] == [16, 16, 8, 8, 4, 4]
    assert 4 * (31 + 2) * 512 == 67584 and 4 * (32 + 2) * 512 == 69632 and 8 * (25 + 2) * 512 == 110592


@pytest.mark.parametrize("G,S", GRADIENT_CASES + FORWARD_CASES)
def test_rt_cases_move_with_the_upper_g_and_the_last_gas(oracle, G, S):
    """The restated CIRSrad agrees with the oracle's own (1e-12: other sums, the same formulas).  With the weights of g >= 24
    zeroed, SPECOUT, dTSURF and every parameter slab that has a merge slot move by at least 1e-4 of their largest element; with
    the last gas slot of dk zeroed, that gas's parameter slab does."""
    c = _case(oracle, G, S)
    spec, dspec, dts = _gradient_oracle(oracle, c)
    np.testing.assert_allclose(c["spec"], spec, rtol=1e-13)
    rs, rd, rt = _restated(oracle, c)
    np.testing.assert_allclose(rs, spec, rtol=1e-12)
    np.testing.assert_allclose(rt, dts, rtol=1e-12)
    assert _slab_err(rd, dspec).max() < 1e-12
    slots = list(c["igas_map"]) + [c["NVMR"]]
    if G > 24:
        ws, wd, wt = _restated(oracle, c, weights=_without_upper_g(c))
        print("g >= 24 zeroed: SPECOUT moves by %.2e, dTSURF %.2e, the least of the slabs %.2e of its largest element"
              % (_moves("SPECOUT", ws, spec), _moves("dTSURF", wt, dts), _moves("dSPECOUT", wd[:, slots], dspec[:, slots], (0, 2, 3))))
    last = int(c["igas_map"][S - 1])
    _, ld, _ = _restated(oracle, c, dk=_without_last_gas(_merge(oracle, c)[1]))
    print("last gas slot zeroed: its slab moves by %.2e" % _moves("dSPECOUT", ld[:, last], dspec[:, last]))
    others = [k for k in range(c["NPAR"]) if k != last]
    assert np.array_equal(ld[:, others], rd[:, others])


def test_two_gases_on_one_column_in_the_reference(oracle):
    """igas_map [0, 2, 2, 4]: the oracle's CIRSrad gives parameter 2 to the later gas (its column 2 is the restatement's with gas 1
    left out), parameter 1, which no gas names, has its continuum part alone, and the column moves when gas 1 has it instead"""
    c = _case(oracle, 10, 4, igas_map=(0, 2, 2, 4))
    ref = _gradient_oracle(oracle, c)
    assert _slab_err(_restated(oracle, c, gases={0, 2, 3})[1], ref[1]).max() < 1e-12
    assert np.array_equal(_restated(oracle, c, gases=set())[1][:, 1], _restated(oracle, c)[1][:, 1])
    _moves("column 2", _restated(oracle, c, gases={0, 1, 3})[1][:, 2], ref[1][:, 2])


def _fused_reference(route, c, oracle, weights=None, dk=None, C=None):
    """(spectrum, gradient with the parameter on axis 1) of a fused route's case by its collapsed restatement on the oracle's
    opacities, as the route's _check_case forms it, with the quadrature weights, dk or the mixing matrix replaced"""
    mod = {"transit": ttg, "occultation": tog, "limb": tlg, "disc": tdg}[route]
    tautot, dk0 = (tlg if route == "disc" else mod)._opacities(oracle, c)
    nvmr, npar, ig = mod._dims(c)
    dtau = tc.dtautot(dk0 if dk is None else dk, ig, nvmr, npar, c["dcont"])
    w = np.asarray(c["delg"] if weights is None else weights, dtype=np.float64)
    C = c.get("C") if C is None else C
    if route == "transit":
        ref = tc.collapsed(tautot, w, tc.path_matrix(c["L"], c["NLAYIN"], c["LAYINC"], c["SCALE"]), c["weight"], dtau)
    elif route == "occultation":
        ref = oc.collapsed(tautot, w, tc.path_matrix(c["L"], c["NLAYIN"], c["LAYINC"], c["SCALE"]), C, dtau, c["xfac"])
    elif route == "limb":
        ref = lc.collapsed(tautot, w, c["NLAYIN"], c["LAYINC"], c["SCALE"], c["EMTEMP"], C, 0, c["WAVE"], nvmr, dtau, c["xfac"])
    else:
        ref = dc.collapsed(tautot, w, c["lp"], c["LAYINC"], c["SCALE"], c["EMTEMP"], 180.0, c["emis"], C, 0, c["WAVE"], nvmr, dtau, c["xfac"])
    return ref[0], ref[-1], ig, nvmr


def _fused_size_case(route, G, S):
    return {"transit": ttg, "occultation": tog, "limb": tlg, "disc": tdg}[route]._wide_case(G, S)


@pytest.mark.parametrize("route,G,S", [(r, G, S) for r in ("transit", "occultation", "limb", "disc") for G, S in sorted(tlg.SIZE_CASES)]
                         + [("transit", 20, 16)])
def test_fused_size_cases_move_with_the_upper_g_and_the_last_gas(oracle, route, G, S):
    """The expected AREA / MOD and every parameter slab with a merge slot of each route's size case (and of the transit file's
    G = 20, S = 16 case) move by at least 1e-4 of their largest element when the weights of g >= 24 are zeroed (G > 24), the last
    gas's slab when its slot of dk is zeroed"""
    c = _fused_size_case(route, G, S)
    assert c["S"] == S and c["K"].shape[1] == G and c["K"].shape[-1] == S
    spec, grad, ig, nvmr = _fused_reference(route, c, oracle)
    slots = list(ig) + [nvmr]
    axes = tuple(a for a in range(grad.ndim) if a != 1)
    if G > 24:
        ws, wg, _, _ = _fused_reference(route, c, oracle, weights=_without_upper_g(c))
        print("g >= 24 zeroed: the spectrum moves by %.2e, the least of the slabs %.2e of its largest element"
              % (_moves("spectrum", ws, spec), _moves("gradient", wg[:, slots], grad[:, slots], axes)))
    dk = (tlg if route == "disc" else {"transit": ttg, "occultation": tog, "limb": tlg}[route])._opacities(oracle, c)[1]
    lg = _fused_reference(route, c, oracle, dk=_without_last_gas(dk))[1]
    print("last gas slot zeroed: its slab moves by %.2e" % _moves("gradient", lg[:, ig[S - 1]], grad[:, ig[S - 1]]))


@pytest.mark.parametrize("route", ["occultation", "limb", "disc"])
def test_fused_many_geometry_cases_move_when_geometries_4_and_8_change_places(oracle, route):
    """Row 4 of the mix is empty and row 8 is not, so with the two exchanged MOD and dMOD of both move by all of row 8's; and with
    the last gas slot of dk zeroed that gas's slab moves"""
    c = tdg._case(130, P=9, Q=9) if route == "disc" else {"occultation": tog, "limb": tlg}[route]._case(130, kind="many")
    spec, grad, ig, nvmr = _fused_reference(route, c, oracle)
    swapped = np.array(c["C"])
    swapped[[4, 8]] = swapped[[8, 4]]
    ss, sg, _, _ = _fused_reference(route, c, oracle, C=swapped)
    assert np.array_equal(ss[:, 4], spec[:, 8]) and np.all(ss[:, 8] == 0.0)
    slots = list(ig) + [nvmr]
    _moves("MOD", ss[:, [4, 8]], spec[:, [4, 8]])
    _moves("dMOD", sg[:, slots][..., [4, 8]], grad[:, slots][..., [4, 8]], (0, 2, 3))
    dk = (tlg if route == "disc" else {"occultation": tog, "limb": tlg}[route])._opacities(oracle, c)[1]
    lg = _fused_reference(route, c, oracle, dk=_without_last_gas(dk))[1]
    _moves("gradient", lg[:, ig[-1]], grad[:, ig[-1]])


# ---- the kernels, on the GPU -------------------------------------------------------------------------------------------------------

def _upload(eng, c):
    eng.upload_ktable(c["K"], c["PRESS"], c["TEMP"], c["WAVE"], c["delg"])
    dims, _ = eng.ktable_info()
    assert dims == (W, c["G"], 6, 5, c["S"])


def _gradient_call(eng, c, lp=None, lt=None, am=None, cont=None, dcont=None, n=1):
    rep = lambda a: a if n == 1 else np.repeat(a[None], n, 0)
    return eng.cirsradg_ck_thermal(0, rep(c["lp"]) if lp is None else lp, rep(c["lt"]) if lt is None else lt, rep(c["am"]) if am is None else am,
                                   rep(c["cont"]), rep(c["dcont"]), c["NVMR"], c["NPAR"], c["igas_map"], c["NLAYIN"], c["LAYINC"], c["SCALE"],
                                   c["EMTEMP"], TSURF, EMISSIVITY=c["emis"], xfac=c["xfac"])


def _compare_gradient(what, got, ref):
    (spec, dspec, dts), (rs, rd, rt) = got, ref
    err = _slab_err(dspec, rd)
    print("%s: SPECOUT rel %.3e, dTSURF rel %.3e, dSPECOUT %.3e of a parameter slab's largest element"
          % (what, np.max(np.abs(spec / rs - 1.0)), np.max(np.abs(dts / rt - 1.0)), err.max()))
    np.testing.assert_allclose(spec, rs, rtol=1e-10)
    np.testing.assert_allclose(dts, rt, rtol=1e-10, atol=0)
    assert err.max() < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("G,S", GRADIENT_CASES, ids=["G%d-S%d-GY%d" % (G, S, launch_rtg_groups(S + 1)) for G, S in GRADIENT_CASES])
def test_gradient_rt_builds_vs_oracle(eng, oracle, G, S):
    """cirsradg_ck_thermal against the oracle's CIRSrad(return_grad=True) on both sides of each build rule of launch_rtg:
    NP1 = 14 (the last of GY 16, both register slots at G = 32), 15 and 30 (the first and last of GY 8, all four slots), 31 and 32
    (GY 4, all eight slots, 67 584 and 69 632 B of LDS; at S = 31 gas 30 and the temperature on bits 30 and 31 of the mask),
    G = 3 (fewer g-ordinates than g-groups) and G = 25 (just past 24).  At (32, 31) also a two-model batch whose second model has
    one amount set to zero (the skip rules), and cirsradg_ck_transmission on the same path against the restatement of
    test_cirsradg_transmission_vs_oracle."""
    c = _case(oracle, G, S)
    _upload(eng, c)
    ref = _gradient_oracle(oracle, c)
    _compare_gradient("G = %d, S = %d" % (G, S), _gradient_call(eng, c), ref)
    if (G, S) != (32, 31):
        return
    am = np.repeat(c["am"][None], 2, 0)
    am[1, 1, 3] = 0.0
    got = _gradient_call(eng, c, am=am, n=2)
    _compare_gradient("model 0 of 2", [a[0] for a in got], ref)
    _compare_gradient("model 1 of 2, an amount of zero", [a[1] for a in got], _gradient_oracle(oracle, c, amount=am[1]))
    # the transmission branch: dSPECOUT = -SPECOUT dTAUTOT_LAYINC (:4128-4131), restated on the oracle's merge
    solflux = np.linspace(1.0e-8, 1.0e-7, W)
    spec, dspec = eng.cirsradg_ck_transmission(c["lp"], c["lt"], c["am"], c["cont"], c["dcont"], c["NVMR"], c["NPAR"], c["igas_map"],
                                               c["NLAYIN"], c["LAYINC"], c["SCALE"], xfac=solflux)
    tau, dk = _merge(oracle, c)
    dtau = tc.dtautot(dk, c["igas_map"], c["NVMR"], c["NPAR"], c["dcont"])
    sg = np.exp(-np.sum((tau + c["cont"][:, None, :])[:, :, c["LAYINC"]] * c["SCALE"], axis=2)) * solflux[:, None, None]         # (W, G, P)
    delg = np.asarray(c["delg"], dtype=np.float64)
    dref = np.nan_to_num(np.tensordot(-sg[:, :, None, None, :] * (dtau[:, :, :, c["LAYINC"]] * c["SCALE"]), delg, axes=([1], [0])))
    scale = np.max(np.abs(dref), axis=(0, 2), keepdims=True)
    err = np.max(np.abs(dspec - dref) / np.where(scale > 0, scale, 1.0))
    print("transmission: SPECOUT rel %.3e, dSPECOUT %.3e" % (np.max(np.abs(spec / np.tensordot(sg, delg, axes=([1], [0])) - 1.0)), err))
    np.testing.assert_allclose(spec, np.tensordot(sg, delg, axes=([1], [0])), rtol=1e-11)
    assert np.all(scale > 0) and err < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("G,S", FORWARD_CASES)
def test_forward_rt_builds_vs_oracle(eng, oracle, G, S):
    """cirsrad_ck_thermal with g-ordinates in register slot 3 (g >= 24) of every build of k_thermal_rt, each model of each call
    against the oracle: one model (<false>); five models with de-duplication off (<true>); the same five with it on
    (<false, 1> for state 0, which writes the prefix records, and <true, 2> for the others, which read them) -- states that
    differ from state 0 in one layer near the top, in one layer near the bottom, in the continuum only, and in nothing."""
    c = _case(oracle, G, S)
    _upload(eng, c)
    n = 5
    lp, lt, am, cont = (np.repeat(c[k][None], n, 0) for k in ("lp", "lt", "am", "cont"))
    lt[1, L - 2] *= 1.02                         # near the top: nearly nothing shared on the way down
    am[2, 1, 1] *= 1.05                          # near the bottom: most of the path shared
    cont[3, :, 4] *= 1.01                        # the continuum alone; state 4: nothing changed
    EMTEMP = lt[:, c["LAYINC"][:, 0]][:, :, None]
    tsurf = np.full(n, TSURF)
    ref = [c["spec"]] + [_forward_oracle(oracle, c, amount=am[m], lt=lt[m], cont=cont[m]) for m in range(1, n)]
    assert np.array_equal(ref[4], ref[0]) and not any(np.array_equal(ref[m], ref[0]) for m in (1, 2, 3))
    call = lambda s: eng.cirsrad_ck_thermal(0, lp[s], lt[s], am[s], cont[s], c["NLAYIN"], c["LAYINC"], c["SCALE"], EMTEMP[s], tsurf[s],
                                            EMISSIVITY=c["emis"], xfac=c["xfac"])
    one = call(slice(0, 1))
    assert not eng.last_rt_shared()
    eng.set_layer_dedup(False)
    try:
        plain = call(slice(None))
        assert not eng.last_rt_shared()
    finally:
        eng.set_layer_dedup(True)
    shared = call(slice(None))
    assert eng.last_rt_shared()
    for what, out in (("one model", one), ("five models", plain), ("five models, shared prefix", shared)):
        print("%s: SPECOUT rel %s" % (what, np.array2string(np.array([np.max(np.abs(o / r - 1.0)) for o, r in zip(out, ref)]), precision=2)))
    for what, out in (("one model", one), ("five models", plain), ("five models, shared prefix", shared)):
        for m in range(out.shape[0]):
            np.testing.assert_allclose(out[m], ref[m], rtol=1e-10, atol=0, err_msg="%s, model %d" % (what, m))
    assert np.array_equal(shared, plain) and np.array_equal(shared[4], shared[0])


@pytest.mark.gpu
def test_gas_selection_at_the_top_of_the_mask(eng, oracle):
    """G = 32, S = 31: gases {0, 30} with the temperature (bits 0, 30 and 31), then gas 30 alone without it (bit 30 only).  Against
    the oracle with the deselected slots removed from dTAUTOT; the selected parameters equal the unmasked run bit for bit."""
    c = _case(oracle, 32, 31)
    _upload(eng, c)
    full = _gradient_call(eng, c)
    _compare_gradient("all gases", full, _gradient_oracle(oracle, c))
    ig, NVMR = c["igas_map"], c["NVMR"]
    try:
        for gases, temperature in (([0, 30], True), ([30], False)):
            eng.set_gradient_gases(gases, temperature=temperature)
            part = _gradient_call(eng, c)
            _compare_gradient("gases %s, temperature %s" % (gases, temperature), part,
                              _restated(oracle, c, gases=set(gases), temperature=temperature))
            assert np.array_equal(part[0], full[0]) and np.array_equal(part[2], full[2])
            for i in gases:
                assert np.array_equal(part[1][:, ig[i]], full[1][:, ig[i]]), i
            assert np.array_equal(part[1][:, NVMR], full[1][:, NVMR]) == temperature
            for i in set(range(31)) - set(gases):                      # switched off: the continuum part alone
                assert not np.array_equal(part[1][:, ig[i]], full[1][:, ig[i]]), i
    finally:
        eng.set_gradient_gases(None)
    assert np.array_equal(_gradient_call(eng, c)[1], full[1])


@pytest.mark.gpu
def test_two_gases_on_one_column(eng, oracle):
    """S = 4 with igas_map [0, 2, 2, 4]: gases 1 and 2 name parameter 2, and the later one has it (the assignment order of
    :3868-3870, which the oracle's CIRSrad follows: its column 2 is gas 2's).  With gas 2 deselected, gas 1 keeps the column."""
    c = _case(oracle, 10, 4, igas_map=(0, 2, 2, 4))
    _upload(eng, c)
    ref = _gradient_oracle(oracle, c)
    later = _restated(oracle, c, gases={0, 2, 3})
    assert _slab_err(later[1], ref[1]).max() < 1e-12                    # the oracle's column 2 carries gas 2 alone
    got = _gradient_call(eng, c)
    _compare_gradient("igas_map [0, 2, 2, 4]", got, ref)
    earlier = _restated(oracle, c, gases={0, 1, 3})
    _moves("column 2", earlier[1][:, 2], ref[1][:, 2])
    try:
        eng.set_gradient_gases([0, 1, 3])
        part = _gradient_call(eng, c)
    finally:
        eng.set_gradient_gases(None)
    _compare_gradient("gas 2 deselected", part, earlier)
    for par in (0, 4, c["NVMR"]):
        assert np.array_equal(part[1][:, par], got[1][:, par])


@pytest.mark.gpu
def test_gas_count_edges(eng, oracle):
    """S = 33 without gradients runs and agrees with the oracle.  S = 32 with gradients is beyond the gas mask (bit 31 is the
    temperature's): the six gradient entries refuse it with the library's own message -- refusals of arguments by host code,
    before anything is launched on them -- and the engine goes on: a valid call after them agrees with the oracle."""
    c = _case(oracle, 10, 33)
    _upload(eng, c)
    out = eng.cirsrad_ck_thermal(0, c["lp"], c["lt"], c["am"], c["cont"], c["NLAYIN"], c["LAYINC"], c["SCALE"], c["EMTEMP"], TSURF,
                                 EMISSIVITY=c["emis"], xfac=c["xfac"])
    print("S = 33: SPECOUT rel %.3e" % np.max(np.abs(out / c["spec"] - 1.0)))
    np.testing.assert_allclose(out, c["spec"], rtol=1e-10, atol=0)
    c = _case(oracle, 10, 32)
    _upload(eng, c)
    out = eng.cirsrad_ck_thermal(0, c["lp"], c["lt"], c["am"], c["cont"], c["NLAYIN"], c["LAYINC"], c["SCALE"], c["EMTEMP"], TSURF,
                                 EMISSIVITY=c["emis"], xfac=c["xfac"])
    np.testing.assert_allclose(out, c["spec"], rtol=1e-10, atol=0)
    layers = (c["lp"], c["lt"], c["am"], c["cont"], c["dcont"], c["NVMR"], c["NPAR"], c["igas_map"])
    nadir = (c["NLAYIN"], c["LAYINC"], c["SCALE"])
    limb = tc.limb_paths(L, np.random.default_rng(5))
    P = limb[0].size
    mix = np.full((1, P), 1.0 / P)
    emtemp = np.where(np.arange(2 * L)[:, None] < limb[0][None, :], c["lt"][limb[1]], 0.0)
    entries = {
        "thermal": lambda: eng.cirsradg_ck_thermal(0, *layers, *nadir, c["EMTEMP"], TSURF, EMISSIVITY=c["emis"]),
        "transmission": lambda: eng.cirsradg_ck_transmission(*layers, *nadir),
        "transit": lambda: eng.cirsradg_ck_transit(*layers, *limb, np.ones(P)),
        "occultation": lambda: eng.cirsradg_ck_occultation(*layers, *limb, mix),
        "limb": lambda: eng.cirsradg_ck_limb(0, *layers, *limb, emtemp, mix),
        "disc": lambda: eng.cirsradg_ck_disc(0, *layers, c["LAYINC"][:, 0], c["SCALE"], c["EMTEMP"][:, 0], TSURF, EMISSIVITY=c["emis"],
                                             mix=np.ones((1, 1))),
    }
    for name, call in entries.items():
        with pytest.raises(NotImplementedError, match="at most 31 spectroscopic gases"):
            call()
    c = _case(oracle, 25, 3)
    _upload(eng, c)
    _compare_gradient("after the refusals", _gradient_call(eng, c), _gradient_oracle(oracle, c))
