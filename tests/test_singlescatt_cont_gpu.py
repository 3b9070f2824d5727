"""The continuum, the scattering opacity and the layer-mean phase functions of a single-scattering Jacobian batch formed inside the
batched call, per distinct layer, from the sources resident in the context (ansfm_cirsrad_ck_singlescatt_batch_cont,
k_ss_cont_rows, the by-row builds of k_thermal_rt): bit identity with ansfm_cirsrad_ck_singlescatt_batch on dense arrays formed in
NumPy from calc_tau_cia / calc_tau_dust / calc_tau_rayleigh with the reference's lines (singlescatt_cont_cases), the sharing with
state 0, the refusals and the model level (scatter_state.BatchedCKSingleScatterModel).  Every comparison is np.array_equal."""
import os

import numpy as np
import pytest

import singlescatt_cases as sc
import singlescatt_cont_cases as cc
from singlescatt_cont_cases import L, P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "tau_cia.npz"))


def check(eng, c, singles=False):
    """fused == the dense batch entry (== n single calls); the rows and the sharing as counted by hand -> the spectra"""
    cc.upload(eng, c)
    eng.set_layer_dedup(True)
    d = cc.dense_arrays(eng, c)
    ref = cc.dense_batch(eng, c, d)
    n = c["n"]
    assert ref.shape == (n, c["W"], P) and np.all(np.isfinite(ref)) and np.all(ref > 0)
    got = cc.fused(eng, c)
    assert np.array_equal(got, ref)
    assert eng.last_layer_rows() == ((cc.distinct_rows(c) if n > 1 else L), n * L)
    assert eng.last_rt_shared() == (n >= 4)
    if singles:
        b = c["b"]
        for m in range(n):
            one = eng.cirsrad_ck_singlescatt(c["ISPACE"], b["PRESS"][m], b["TEMP"][m], b["amount"][m], d[0][m], d[1][m], d[2][m],
                                             c["base"]["NLAYIN"], c["base"]["LAYINC"], c["SCALE"][m], c["EMTEMP"][m], float(b["TSURF"][m]),
                                             c["base"]["EMIS"], c["base"]["BRDF"], c["base"]["SOLF"], c["base"]["sol"], c["base"]["emi"],
                                             xfac=c["base"]["xfac"])
            assert np.array_equal(got[m], one), m
    return got, d


# ---- 1. fused == dense batch entry == n single calls --------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ISPACE", [("sorted", 0), ("scrambled", 0), ("lbl", 0), ("sorted", 1)])
def test_fused_equals_the_dense_entry_and_single_calls(eng, golden, kind, ISPACE):
    c = cc.case(golden, kind=kind, ISPACE=ISPACE)
    got, d = check(eng, c, singles=True)
    assert cc.distinct_rows(c) == L + 5                        # states 1, 2, 3, 4 and 7 differ in one layer each
    # every state's spectrum differs from state 0's except the one that differs in nothing
    for m in range(1, c["n"]):
        assert np.array_equal(got[m], got[0]) == (m == 6), m
    assert np.all(d[2][:, :, :, cc.EMPTY_LAYER] > 0)          # Rayleigh scattering alone in the layer without aerosol


# ---- 2. term subsets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cia,NDUST,IRAY", [(False, 2, 0), (False, 0, 1), (False, 2, 1), (True, 2, 0), (True, 2, 1)])
def test_term_subsets_against_their_dense_twins(eng, golden, cia, NDUST, IRAY):
    c = cc.case(golden, cia=cia, NDUST=NDUST, IRAY=IRAY)
    got, d = check(eng, c)
    assert (d[0] is not None) and d[0].shape == d[1].shape
    if IRAY == 0:                                               # the layer without aerosol: num = 0 and nothing is divided
        assert not d[2][:, :, :, cc.EMPTY_LAYER].any() and not d[1][:, :, cc.EMPTY_LAYER].any()
    want = L + 2 + 1 + (NDUST > 0) + (1 if cia else 0)         # TEMP twice, TOTAM (through the amounts), CONT, He
    assert cc.distinct_rows(c) == want


# ---- 3. below and above the sharing threshold, de-duplication on and off ----------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_number_of_states_and_deduplication(eng, golden, n):
    c = cc.case(golden, n=n)
    got, d = check(eng, c)
    assert cc.distinct_rows(c) == L + [0, 1, 2, 5][[1, 2, 3, 8].index(n)]
    try:
        eng.set_layer_dedup(False)
        assert np.array_equal(cc.fused(eng, c), got)
        assert eng.last_layer_rows() == (n * L, n * L) and eng.last_rt_shared() is False
    finally:
        eng.set_layer_dedup(True)
    assert np.array_equal(cc.fused(eng, c), got) and eng.last_rt_shared() == (n >= 4)


# ---- 4. seven populations: eight terms in the phase sum ---------------------------------------------------------------------
def test_seven_populations(eng, golden):
    c = cc.case(golden, NDUST=7)
    check(eng, c)


# ---- 5. a full tile and one wavenumber more -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [64, 65])
def test_tile_edge(eng, golden, W):
    check(eng, cc.case(golden, W=W))


# ---- 6. the model ---------------------------------------------------------------------------------------------------------------
def test_batched_singlescatt_model_fused_dense_and_jacobian(golden):
    import archnemesis_dist_amd as pkg
    from archnemesis_dist_amd import synthetic as syn
    from archnemesis_dist_amd.jacobian import finite_difference_jacobian, jacobian_nemesis_batched, perturbed_states
    from archnemesis_dist_amd.profile_state import ContinuousProfileState
    from archnemesis_dist_amd.scatter_state import BatchedCKSingleScatterModel
    from test_continuum_fused_gpu import cia_tables, dust_table
    NPRO, NLAY, W = 10, 12, 70
    t = sc.synthetic_table("sorted", W, cc.G, 4)
    t["WAVE"] = cc.grid(0, W)
    rng = np.random.default_rng(77)
    pr = syn.synth_profiles(NPRO, cc.NVMR, seed=5, p_bottom_bar=5.0, p_top_bar=1.0e-5)
    DUST = 1.0e3 * np.exp(-np.linspace(0.0, 4.0, NPRO))[:, None] * np.array([1.0, 0.3])[None]
    st = ContinuousProfileState(pr["H"], pr["P"], pr["T"], pr["VMR"], ["T", ("VMR", 2), ("DUST", 0)], DUST=DUST)
    SWAVE, KEXT, KSCA = dust_table(t["WAVE"], 2)
    eng = pkg.AnsfmEngine(0)
    try:
        sc.upload(eng, t)
        model = BatchedCKSingleScatterModel(eng, st, pr["RADIUS"], pr["ID"], pr["ISO"], [2, 3, 4, 5],
                                            10.0 ** rng.uniform(-1.5, 0.3, (W, 1, 3)), [30.0], [20.0], 10.0 ** rng.uniform(-8, -7, W),
                                            layering_args=dict(NLAY=NLAY, LAYINT=1, NINT=101), geometry=dict(ANGLE=20.0, EMISS_ANG=20.0),
                                            IRAY=1, cia=dict(zip(cc.CIA_NAMES, cia_tables(golden, "normal"))),
                                            dust=dict(SWAVE=SWAVE, KEXT=KEXT, KSCA=KSCA), BRDF=rng.uniform(0.02, 0.15, (W, 1)), TSURF=150.0,
                                            emissivity=rng.uniform(0.7, 1.0, W), xfac=rng.uniform(0.5, 2.0, W))
        assert model.fused_continuum is True and model.ny() == W
        st.calc_DSTEP()
        X = np.ascontiguousarray(perturbed_states(st.XN, st.DSTEP).T)
        Y = model.spectra_batch(X).cpu().numpy()
        rows, total = model.last_rows
        assert total == (st.NX + 1) * NLAY and NLAY < rows < total // 2 and model.last_shared is True
        assert Y.shape == (st.NX + 1, W) and np.all(np.isfinite(Y))
        model.fused_continuum = False
        Y_d = model.spectra_batch(X).cpu().numpy()
        assert np.array_equal(Y, Y_d)
        model.fused_continuum = True
        YN, KK = jacobian_nemesis_batched(model)
        YN_q, KK_q = finite_difference_jacobian(np.ascontiguousarray(Y.T), st.XN, np.arange(st.NX))
        assert np.array_equal(YN, YN_q) and np.array_equal(KK, KK_q)
        assert KK.shape == (W, 3 * NPRO) and np.all(np.any(KK != 0.0, axis=0))     # every element reaches the spectrum
    finally:
        eng.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_context_goes_on(golden):
    import archnemesis_dist_amd as pkg
    e = pkg.AnsfmEngine(0)
    try:
        c = cc.case(golden)
        b = c["b"]
        sc.upload(e, c["t"])
        with pytest.raises(ValueError, match="INVALID"):                     # CIA before upload_cia
            cc.fused(e, c)
        e.upload_cia(0, c["t"]["WAVE"], *c["tabs"], b["ID"], b["ISO"])
        with pytest.raises(ValueError, match="INVALID"):                     # aerosols before upload_dust
            cc.fused(e, c)
        e.upload_dust(c["dust"]["SWAVE"], c["dust"]["KEXT"], c["dust"]["KSCA"])
        good = cc.fused(e, c)
        assert good.shape == (c["n"], c["W"], P) and np.all(np.isfinite(good))
        sc.upload(e, c["t"])                                                 # a new table clears the sources
        with pytest.raises(ValueError, match="INVALID"):
            cc.fused(e, c)
        cc.upload(e, c)
        assert np.array_equal(cc.fused(e, c), good)
        with pytest.raises(ValueError, match="INVALID"):                     # the CIA source is ISPACE 0's
            cc.fused(e, c, ISPACE=1)
        with pytest.raises(ValueError, match="INVALID"):                     # one population given, two uploaded
            cc.fused(e, c, CONT=np.ascontiguousarray(b["CONT"][:, :, :1]), phase_fn=np.ascontiguousarray(c["phase_fn"][:, :, :2]))
        with pytest.raises(ValueError, match="INVALID"):                     # neither aerosols nor Rayleigh: no scattering opacity
            cc.fused(e, c, CONT=None, IRAY=0, phase_fn=np.ascontiguousarray(c["phase_fn"][:, :, :1]))
        with pytest.raises(ValueError):                                      # a used term's array, phase_fn: not given
            cc.fused(e, c, TOTAM=None)
        with pytest.raises(ValueError):
            cc.fused(e, c, FRAC=None)
        with pytest.raises(ValueError):
            cc.fused(e, c, phase_fn=None)
        with pytest.raises(ValueError):                                      # IRAY 4 without the composition
            cc.fused(e, c, IRAY=4)
        with pytest.raises(NotImplementedError, match="7"):                  # eight populations: refused at the upload already
            e.upload_dust(c["dust"]["SWAVE"], np.repeat(c["dust"]["KEXT"], 4, 1), np.repeat(c["dust"]["KSCA"], 4, 1))
        with pytest.raises(NotImplementedError, match="UNSUPPORTED"):        # ... and by the entry, whatever is resident
            cc.fused(e, c, CONT=np.repeat(b["CONT"], 4, 2), phase_fn=np.repeat(c["phase_fn"], 3, 2))
        assert np.array_equal(cc.fused(e, c), good)
        # the dense entry's own reasons: a surface temperature without an emissivity, n_models * P > 65535
        tail = list(cc.rt_tail(c))
        args = (0, b["PRESS"], b["TEMP"], b["amount"], b["q"], b["FRAC"], b["TOTAM"], b["DELH"], b["CONT"], 1, None, c["phase_fn"])
        with pytest.raises(ValueError, match="INVALID"):
            e.cirsrad_ck_singlescatt_batch_cont(*args, *tail[:5], None, *tail[6:])
        big = 32768
        one = lambda a: np.broadcast_to(a[:1], (big,) + a.shape[1:])
        with pytest.raises(NotImplementedError, match="UNSUPPORTED"):
            e.cirsrad_ck_singlescatt_batch_cont(0, *(one(b[k]) for k in ("PRESS", "TEMP", "amount", "q", "FRAC", "TOTAM", "DELH", "CONT")),
                                                1, None, c["phase_fn"], tail[0], tail[1], one(tail[2]), one(tail[3]), one(tail[4]), *tail[5:])
        assert np.array_equal(cc.fused(e, c), good)
    finally:
        e.close()
