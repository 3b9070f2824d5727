"""The continuum of a multiple-scattering Jacobian batch formed inside the batched call, per distinct layer, from the sources
resident in the context (ansfm_upload_cia / ansfm_upload_dust / ansfm_cirsrad_ck_scatter_batch_cont, k_ms_cont_rows): bit
identity with the by-hand route (calc_tau_cia / calc_tau_dust / calc_tau_rayleigh_batch_dev over all N * L layers, ContinuumRows,
cirsrad_ck_scatter_batch_rows), slices, the oracle, the refusals and the model level (scatter_state.BatchedCKScatterModel).

A layer's identity columns are the columns its opacities are formed from: pressure, temperature, the gas amounts, the mixing
ratios, TOTAM, DELH, the aerosol columns with aerosols, the Rayleigh composition at IRAY 4 and the para-H2 fraction for a CIA
table that has a para-H2 axis.  Without that axis the fraction changes no opacity; it is left out so that the layer still counts
as model 0's, as it does in the by-hand route, whose packer compares the opacities themselves."""
import inspect
import os
import re

import numpy as np
import pytest

from test_continuum_fused_gpu import cia_tables, dust_table, grid
from test_gpu_parity import _scatter_inputs, _scatter_oracle, _scatter_vs_oracle
from test_scatter_wavenumber_shard import _ktable_upload

pytestmark = pytest.mark.gpu

W, G, S, L, NVMR, N = 150, 4, 3, 12, 6, 6          # W = 150 is no multiple of the wavenumber tile
CIA_NAMES = ("CIA_WAVEN", "CIA_TEMP", "CIA_FRAC", "NPARA", "K_CIA", "IPAIRG1", "IPAIRG2", "INORMALT", "INORMAL", "INORMALD")
SOL, AZI = np.array([30.0, 120.0]), np.array([45.0, 0.0])
EMI = {False: np.array([20.0, 50.0]), True: np.array([160.0, 130.0])}


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "tau_cia.npz"))


def batch(z, NDUST, n=N, seed=3, negative=False):
    """n states of L = 12 layers (the golden file's nine, interpolated): every state after the first differs from it in exactly
    one layer -- in temperature, only in He's mixing ratio, only in DELH, only in the para-H2 fraction, only in one aerosol
    column -- as test_continuum_fused_gpu.batch builds them.  negative: the second aerosol column of layer 1 is so negative
    that TAUSCAT of the layer is below zero at every wavenumber."""
    from archnemesis_dist_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    ID, ISO = syn.PROFILE_GAS_ID[:NVMR].copy(), np.zeros(NVMR, dtype=np.int32)       # 39, 40, 6, 11, 26, 27
    L0 = z["PRESS"].shape[0]
    ext = lambda a: np.interp(np.linspace(0.0, L0 - 1.0, L), np.arange(L0), np.asarray(a, float))
    rep = lambda a: np.repeat(np.asarray(a, float)[None], n, 0)
    PRESS, TEMP, FRAC, TOTAM, DELH = (rep(ext(z[k])) for k in ("PRESS", "TEMP", "FRAC", "TOTAM", "DELH"))
    q0 = np.empty((L, NVMR))
    q0[:, 2:] = 10.0 ** rng.uniform(-6, -3, (L, NVMR - 2))
    rest = 1.0 - q0[:, 2:].sum(1)
    q0[:, 0], q0[:, 1] = 0.864 * rest, 0.136 * rest
    PP = rep(q0 * PRESS[0][:, None])
    CONT = rep(10.0 ** rng.uniform(8, 10, (L, max(NDUST, 1))))[:, :, :NDUST]
    changes = [lambda: TEMP.__setitem__((1, 3), TEMP[1, 3] * 1.05), lambda: PP.__setitem__((2, 4, 1), PP[2, 4, 1] * 1.05),
               lambda: DELH.__setitem__((3, 2), DELH[3, 2] * 1.05), lambda: FRAC.__setitem__((4, 5), FRAC[4, 5] + 0.03),
               lambda: NDUST and CONT.__setitem__((5, 6, 0), CONT[5, 6, 0] * 1.05)]
    for change in changes[:n - 1]:
        change()
    if negative:
        _, _, KSCA = dust_table(grid(0), NDUST)
        # |CONT_1| min ksca_1 > CONT_0 max ksca_0 with a factor 2 to spare (the spline between the tabulated points)
        CONT[:, 1, 1] = -2.0 * CONT[0, 1, 0] * KSCA[:, 0].max() / KSCA[:, 1].min()
    q = PP / PRESS[:, :, None]
    amount = np.ascontiguousarray(np.transpose(q[:, :, 2:2 + S] * TOTAM[:, :, None], (0, 2, 1))) * 1.0e-4
    return dict(ID=ID, ISO=ISO, PRESS=PRESS, TEMP=TEMP, FRAC=FRAC, TOTAM=TOTAM, DELH=DELH, PP=PP, q=q, CONT=CONT, amount=amount)


def case(golden, tag, ISPACE, IRAY, NDUST, NMU, NF, up=False, lowbc=1, nW=W, n=N, negative=False):
    """the k-table, the scattering inputs that do not depend on the state, the states and their boundary radiances"""
    from archnemesis_dist_amd.scatter_state import planck
    rng = np.random.default_rng(8800 + NMU + 7 * NF + 3 * NDUST + IRAY)
    z = _scatter_inputs(rng, nW, G, L, S, NMU, NF, NDUST, 1, 1 if IRAY else 0, lowbc)
    z["WAVE"] = 100.0 + 20.0 * np.arange(nW) if ISPACE == 0 else np.linspace(1.8, 60.0, nW)     # inside the CIA table: grid()
    b = batch(golden, NDUST, n=n, negative=negative)
    radg = np.stack([np.repeat(planck(ISPACE, z["WAVE"], b["TEMP"][m, 0])[:, None], NMU, 1) for m in range(n)])
    tabs = cia_tables(golden, tag)
    dust = dict(zip(("SWAVE", "KEXT", "KSCA"), dust_table(z["WAVE"], NDUST))) if NDUST else None
    return dict(z=z, b=b, radg=radg, tabs=tabs, cia=dict(zip(CIA_NAMES, tabs)), dust=dust, tag=tag, ISPACE=ISPACE, IRAY=IRAY,
                NDUST=NDUST, NMU=NMU, NF=NF, up=up, lowbc=lowbc, W=nW, n=n)


def upload(eng, c, s=0, t=None):
    """the table's slice [s, t) and, on its grid, the sources"""
    z, b = c["z"], c["b"]
    t = c["W"] if t is None else t
    _ktable_upload(z)(eng, s, t)
    eng.upload_cia(c["ISPACE"], z["WAVE"][s:t], *c["tabs"], b["ID"], b["ISO"])
    if c["NDUST"]:
        eng.upload_dust(c["dust"]["SWAVE"], c["dust"]["KEXT"], c["dust"]["KSCA"])


def tail(c, s=0, t=None, sel=slice(None)):
    """the arguments behind the continuum, alike for the rows entry and the fused one"""
    z = c["z"]
    t = c["W"] if t is None else t
    return (np.ascontiguousarray(c["radg"][sel, s:t]), SOL, EMI[c["up"]], AZI, z["solar"][s:t], c["lowbc"],
            np.ascontiguousarray(z["brdf"][s:t]), z["MU"], z["WT"], c["NF"], 101, c["IRAY"], 1)


def by_hand(eng, c, s=0, t=None, sel=slice(None)):
    """calc_tau_cia / calc_tau_dust / calc_tau_rayleigh_batch_dev over all layers, ContinuumRows, the rows entry"""
    from archnemesis_dist_amd.scatter_state import continuum_rows_by_hand
    b, z = c["b"], c["z"]
    lay = {k: b[k][sel] for k in ("PP", "PRESS", "TEMP", "FRAC", "TOTAM", "DELH", "CONT")}
    pk = continuum_rows_by_hand(eng, c["ISPACE"], c["IRAY"], b["ID"], b["ISO"], c["cia"], c["dust"], lay)
    assert pk.TAUCIA_rows is not None and (pk.TAURAY_rows is None) == (c["IRAY"] == 0) and (pk.TAUSCAT_rows is None) == (c["NDUST"] == 0)
    ws = None if (s == 0 and t is None) else (s, c["W"])
    out = eng.cirsrad_ck_scatter_batch_rows(c["ISPACE"], b["PRESS"][sel], b["TEMP"][sel], b["amount"][sel], pk.cont_row, pk.TAUCIA_rows,
                                            pk.TAUDUST_rows, pk.TAURAY_rows, pk.TAUSCAT_rows, z["phasarr"] if c["NDUST"] else None,
                                            pk.lfrac_rows, *tail(c, s, t, sel), wave_slice=ws)
    return out, pk


def fused(eng, c, s=0, t=None, sel=slice(None), **over):
    b, z = c["b"], c["z"]
    f4 = eng.rayleigh_f4(b["ID"], b["ISO"], b["q"][sel]) if c["IRAY"] == 4 else None
    ws = None if (s == 0 and t is None) else (s, c["W"])
    kw = dict(q=b["q"][sel], FRAC=b["FRAC"][sel], TOTAM=b["TOTAM"][sel], DELH=b["DELH"][sel], CONT=b["CONT"][sel] if c["NDUST"] else None,
              phasarr=z["phasarr"] if c["NDUST"] else None, ISPACE=c["ISPACE"])
    kw.update(over)
    return eng.cirsrad_ck_scatter_batch_cont(kw["ISPACE"], b["PRESS"][sel], b["TEMP"][sel], b["amount"][sel], kw["q"], kw["FRAC"],
                                             kw["TOTAM"], kw["DELH"], kw["CONT"], c["IRAY"], f4, kw["phasarr"], *tail(c, s, t, sel),
                                             wave_slice=ws)


def distinct_rows(eng, c):
    """rows the de-duplication computes: state 0's L and every layer of another state that differs from it in a byte of an
    identity column (the module docstring lists them)"""
    b = c["b"]
    cols = [b["PRESS"], b["TEMP"], np.transpose(b["amount"], (0, 2, 1)), b["q"], b["TOTAM"], b["DELH"]]
    cols += [b["FRAC"]] if c["tag"] == "para" else []
    cols += [b["CONT"]] if c["NDUST"] else []
    cols += [eng.rayleigh_f4(b["ID"], b["ISO"], b["q"])] if c["IRAY"] == 4 else []
    n = c["n"]
    ident = np.concatenate([np.ascontiguousarray(a, dtype=np.float64).reshape(n, L, -1) for a in cols], axis=2)
    by = np.ascontiguousarray(ident).view(np.uint8).reshape(n, L, -1)
    return L + int(np.sum(np.any(by[1:] != by[:1], axis=2)))


def check_bit_identity(eng, c):
    upload(eng, c)
    eng.set_layer_dedup(True)
    ref, pk = by_hand(eng, c)
    hits_ref = eng.last_scatter_cache()
    assert ref.shape == (c["n"], c["W"], 2) and np.all(np.isfinite(ref))
    # every state's spectrum differs from state 0's, except where its layer differs in what the case does not use: the para-H2
    # fraction without a para-H2 axis, an aerosol column without aerosols
    for i in range(1, c["n"]):
        unused = (i == 4 and c["tag"] == "normal") or (i == 5 and not c["NDUST"])
        assert np.array_equal(ref[i], ref[0]) == unused, i
    got = fused(eng, c)
    assert np.array_equal(got, ref)
    want = distinct_rows(eng, c)
    assert want == L + 3 + (c["tag"] == "para") + (c["NDUST"] > 0)
    assert eng.last_layer_rows() == (want, c["n"] * L)
    hits = eng.last_scatter_cache()
    assert hits[1] == hits_ref[1] == (c["n"] - 1) * L and hits[0] >= hits_ref[0] > 0, (hits, hits_ref)
    try:
        eng.set_layer_dedup(False)
        assert np.array_equal(fused(eng, c), ref)
        assert eng.last_layer_rows() == (c["n"] * L, c["n"] * L) and eng.last_scatter_cache() == (0, c["n"] * L)
    finally:
        eng.set_layer_dedup(True)
    for i in (0, 2):                                   # one state per call: the model-by-model route
        assert np.array_equal(fused(eng, c, sel=slice(i, i + 1))[0], ref[i])


# ---- 1. bit identity with the rows entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("NMU,NF", [(5, 2), (16, 3)])           # lane kernel, matrix-core chains
@pytest.mark.parametrize("NDUST", [0, 2])
@pytest.mark.parametrize("IRAY", [0, 1, 4])
@pytest.mark.parametrize("tag", ["normal", "para"])
def test_fused_continuum_is_bit_identical_with_the_rows_entry(eng, golden, tag, IRAY, NDUST, NMU, NF):
    check_bit_identity(eng, case(golden, tag, 0, IRAY, NDUST, NMU, NF))


def test_fused_continuum_on_a_wavelength_grid(eng, golden):
    check_bit_identity(eng, case(golden, "para", 1, 4, 2, 5, 2))


def test_layer_cache_switched_off(eng, golden, monkeypatch):
    c = case(golden, "para", 0, 1, 2, 16, 3)
    upload(eng, c)
    ref, _ = by_hand(eng, c)
    monkeypatch.setenv("ANSFM_MS_LAYER_CACHE", "0")
    assert np.array_equal(fused(eng, c), ref)
    assert eng.last_scatter_cache() == (0, N * L)


# ---- 2. a negative aerosol column ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NMU,NF", [(5, 2), (16, 3)])
def test_negative_aerosol_column(eng, golden, NMU, NF):
    """TAUSCAT of layer 1 is negative at every wavenumber: the clip of TAUDUST, the TAUSCAT > 0 guard of the fractions and the
    clamp of the single-scattering albedo; finite by construction"""
    c = case(golden, "para", 0, 1, 2, NMU, NF, negative=True)
    upload(eng, c)
    ref, pk = by_hand(eng, c)
    assert np.all(pk.TAUSCAT_rows[1] < 0.0) and np.all(pk.lfrac_rows[1] == 0.0) and np.all(pk.TAUDUST_rows[1] > 0.0)
    assert np.all(np.isfinite(ref))
    assert np.array_equal(fused(eng, c), ref)
    assert eng.last_layer_rows() == (distinct_rows(eng, c), N * L)


# ---- 3. eight streams, padded to sixteen --------------------------------------------------------------------------------------
def test_eight_streams_padded_to_sixteen(eng, golden):
    c = case(golden, "normal", 0, 1, 2, 8, 2)
    upload(eng, c)
    ref, _ = by_hand(eng, c)
    assert np.all(np.isfinite(ref))
    assert np.array_equal(fused(eng, c), ref)


# ---- 4. slices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NMU,NF", [(5, 2), (16, 3)])
def test_slices_side_by_side_equal_the_whole_axis(eng, golden, NMU, NF):
    """W = 241 cut at 97: the sources are uploaded again on every slice's table"""
    c = case(golden, "para", 0, 4, 2, NMU, NF, nW=241)
    upload(eng, c)
    whole = fused(eng, c)
    hits = eng.last_scatter_cache()
    ref, _ = by_hand(eng, c)
    assert np.array_equal(whole, ref)
    parts = []
    for s, t in ((0, 97), (97, 241)):
        upload(eng, c, s, t)
        parts.append(fused(eng, c, s, t))
        assert parts[-1].shape == (N, t - s, 2) and eng.last_scatter_cache() == hits
    assert np.array_equal(np.concatenate(parts, axis=1), whole)


# ---- 5. models that share every layer with model 0 -----------------------------------------------------------------------------
@pytest.mark.parametrize("NMU,NF", [(5, 2), (16, 3)])
@pytest.mark.parametrize("up", [False, True])
def test_a_model_identical_to_model_0(eng, golden, NMU, NF, up):
    """L = 12 is a multiple of the prefix step: the second model starts its adding sweep behind the last layer"""
    c = case(golden, "para", 0, 1, 2, NMU, NF, up=up, n=1)
    upload(eng, c)
    single = fused(eng, c)
    assert single.shape == (1, W, 2) and np.all(np.isfinite(single))
    two = dict(c, n=2, radg=np.repeat(c["radg"], 2, 0), b={k: (np.repeat(v, 2, 0) if k not in ("ID", "ISO") else v)
                                                           for k, v in c["b"].items()})
    got = fused(eng, two)
    assert eng.last_layer_rows() == (L, 2 * L) and eng.last_scatter_cache() == (L, L)
    assert np.array_equal(got[0], single[0]) and np.array_equal(got[1], single[0])


# ---- 6. the oracle ------------------------------------------------------------------------------------------------------------
def test_fused_continuum_against_the_oracle(eng, oracle, golden):
    """per state: oracle.calc_tau_cia + calc_tau_dust + calc_tau_rayleigh feed the oracle's scattering chain; the bound is the
    one test_gpu_parity._scatter_vs_oracle puts on the g-integrated radiance"""
    m = re.search(r"np\.max\(np\.abs\(out - ref\)\) / np\.max\(np\.abs\(ref\)\) < ([0-9.eE+-]+)", inspect.getsource(_scatter_vs_oracle))
    bound = float(m.group(1))
    c = case(golden, "para", 0, 4, 2, 5, 2)
    upload(eng, c)
    got = fused(eng, c)
    z, b = c["z"], c["b"]
    for i in range(N):
        cia = oracle.calc_tau_cia(0, z["WAVE"], *c["tabs"], b["ID"], b["ISO"], b["PP"][i], b["PRESS"][i], b["TEMP"][i], b["FRAC"][i],
                                  b["TOTAM"][i], b["DELH"][i])[0]
        td1, tcs = oracle.calc_tau_dust(z["WAVE"], c["dust"]["SWAVE"], c["dust"]["KEXT"], c["dust"]["KSCA"], b["CONT"][i])[:2]
        ray = oracle.calc_tau_rayleigh(4, 0, z["WAVE"], b["TOTAM"][i], ID=b["ID"], ISO=b["ISO"], VMR=b["q"][i])[0]
        sca = np.sum(tcs, 2)
        frac = np.where((sca > 0)[:, :, None], tcs / np.where(sca > 0, sca, 1.0)[:, :, None], 0.0)
        zi = dict(z, lay_p=b["PRESS"][i], lay_t=b["TEMP"][i], amount=b["amount"][i], TAUCIA=cia,
                  TAUDUST=np.sum(np.clip(np.nan_to_num(td1), 0, 1e20), 2), TAURAY=ray, TAUSCAT=sca,
                  lfrac=np.ascontiguousarray(np.transpose(frac, (0, 2, 1))), radg=c["radg"][i])
        ref, _, _ = _scatter_oracle(oracle, zi, SOL, EMI[False], AZI, c["lowbc"], c["NF"], 101, 4, 1)
        err = np.max(np.abs(got[i] - ref)) / np.max(np.abs(ref))
        print(f"state {i}: fused continuum vs the oracle chain: {err:.3e} of the largest radiance (bound {bound:g})")
        assert err < bound


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_context_goes_on(golden):
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    try:
        c = case(golden, "normal", 0, 1, 2, 5, 2)
        z, b = c["z"], c["b"]
        _ktable_upload(z)(e, 0, W)
        with pytest.raises(ValueError, match="INVALID"):                     # CIA before upload_cia
            fused(e, c)
        e.upload_cia(0, z["WAVE"], *c["tabs"], b["ID"], b["ISO"])
        with pytest.raises(ValueError, match="INVALID"):                     # aerosols before upload_dust
            fused(e, c)
        e.upload_dust(c["dust"]["SWAVE"], c["dust"]["KEXT"], c["dust"]["KSCA"])
        good = fused(e, c)
        assert good.shape == (N, W, 2) and np.all(np.isfinite(good))
        _ktable_upload(z)(e, 0, W)                                           # a new table clears the sources
        with pytest.raises(ValueError, match="INVALID"):
            fused(e, c)
        upload(e, c)
        assert np.array_equal(fused(e, c), good)
        with pytest.raises(ValueError, match="INVALID"):                     # the CIA source is ISPACE 0's
            fused(e, c, ISPACE=1)
        assert np.array_equal(fused(e, c), good)
        with pytest.raises(ValueError, match="INVALID"):                     # one phase function, two populations uploaded
            fused(e, c, phasarr=np.ascontiguousarray(z["phasarr"][:1]), CONT=np.ascontiguousarray(b["CONT"][:, :, :1]))
        assert np.array_equal(fused(e, c), good)
        with pytest.raises(ValueError):                                      # shape checks before the call
            fused(e, c, q=b["q"][:, :, :-1])
        with pytest.raises(ValueError):
            fused(e, c, TOTAM=b["TOTAM"][:, :-1])
        with pytest.raises(ValueError):
            fused(e, c, CONT=None)
        assert np.array_equal(fused(e, c), good)
    finally:
        e.close()


# ---- 8. the model ---------------------------------------------------------------------------------------------------------------
def test_batched_scatter_model_fused_by_hand_and_per_state(golden):
    """NPRO = 20, NLAY = 12, blocks T and one aerosol profile, 5 streams: jacobian_nemesis_batched gives the same (YN, KK) bits
    with the fused continuum, by hand and on a side torch stream; a perturbed level costs a few rows; every DUST column of KK
    is non-zero somewhere; every state on its own through cirsrad_ck_scatter agrees to 1e-10, the thermal model test's rtol."""
    import torch
    import archnemesis_dist_amd as pkg
    from archnemesis_dist_amd import synthetic as syn
    from archnemesis_dist_amd.jacobian import jacobian_nemesis_batched, perturbed_states
    from archnemesis_dist_amd.profile_state import ContinuousProfileState
    from archnemesis_dist_amd.scatter_state import BatchedCKScatterModel, continuum_rows_by_hand
    NPRO, NLAY, NMU, NF = 20, 12, 5, 2
    rng = np.random.default_rng(8899)
    z = _scatter_inputs(rng, W, G, NLAY, 4, NMU, NF, 2, 1, 1, 1)
    z["WAVE"] = grid(0)
    pr = syn.synth_profiles(NPRO, NVMR, seed=5, p_bottom_bar=5.0, p_top_bar=1.0e-5)
    DUST = 1.0e3 * np.exp(-np.linspace(0.0, 4.0, NPRO))[:, None] * np.array([1.0, 0.3])[None]
    st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("DUST", 0)], DUST=DUST)
    tabs = cia_tables(golden, "normal")
    SWAVE, KEXT, KSCA = dust_table(z["WAVE"], 2)
    eng = pkg.AnsfmEngine(0)
    try:
        eng.upload_ktable(z["K"], z["TPRESS"], z["TTEMP"], z["WAVE"], z["DELG"])
        model = BatchedCKScatterModel(eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], [2, 3, 4, 5], z["phasarr"], z["MU"], z["WT"], NF, 101,
                                      SOL, EMI[False], AZI, z["solar"], layering_args=dict(NLAY=NLAY, LAYINT=1, NINT=101), IRAY=4, IMIE=1,
                                      cia=dict(zip(CIA_NAMES, tabs)), dust=dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA), LOWBC=1,
                                      brdf_matrix=z["brdf"])
        assert model.fused_continuum is True and model.ny() == 2 * W
        YN, KK = jacobian_nemesis_batched(model)
        rows, total = model.last_rows
        hits, layers = model.last_cache
        model.fused_continuum = False
        YN_d, KK_d = jacobian_nemesis_batched(model)
        assert np.array_equal(YN, YN_d) and np.array_equal(KK, KK_d)
        assert model.last_rows[1] == total and model.last_cache[1] == layers and hits >= model.last_cache[0] > 0
        model.fused_continuum = True
        side = torch.cuda.Stream(device=model.torch_device())
        with torch.cuda.stream(side):
            YN_s, KK_s = jacobian_nemesis_batched(model)
        assert np.array_equal(YN, YN_s) and np.array_equal(KK, KK_s)
        assert total == (st.NX + 1) * NLAY and rows < total // 3 and layers == st.NX * NLAY
        assert YN.shape == (2 * W,) and KK.shape == (2 * W, 2 * NPRO) and np.all(np.isfinite(KK))
        assert np.all(np.any(KK[:, NPRO:] != 0.0, axis=0))             # every level of the aerosol profile reaches the spectrum
        # every state on its own
        st.calc_DSTEP()
        X = np.ascontiguousarray(perturbed_states(st.XN, st.DSTEP).T)
        Y = model.spectra_batch(X).cpu().numpy()
        assert np.array_equal(Y[0], YN)
        lay = model.layers(X)
        radg = model.radg(lay)
        for i in range(X.shape[0]):
            one = {k: lay[k][i:i + 1] for k in ("PP", "PRESS", "TEMP", "FRAC", "TOTAM", "DELH", "CONT")}
            pk = continuum_rows_by_hand(eng, 0, 4, pr["ID"], pr["ISO"], model.cia, model.dust, one)
            cia, dust, ray, sca, lf = pk.expand()
            spec = eng.cirsrad_ck_scatter(0, lay["PRESS"][i], lay["TEMP"][i], lay["amount"][i], cia[0], dust[0], ray[0], sca[0],
                                          z["phasarr"], lf[0], radg[i], SOL, EMI[False], AZI, z["solar"], 1, z["brdf"], z["MU"], z["WT"],
                                          NF, 101, 4, 1)
            np.testing.assert_allclose(Y[i], spec.reshape(-1), rtol=1e-10)
    finally:
        eng.close()
