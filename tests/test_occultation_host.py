"""Solar occultation with gradients, without a GPU: the NumPy restatement (tests/occultation_cases.py) against the reference's
own nemesisSOfmg in tests/golden/occultation_c1.npz (tools/golden/gen_golden_occultation.py), the collapsed form against the
un-collapsed one on ragged paths, occultation.tangent_mix against the restatement, and -- where the reference tree is present --
the adapter's nemesisSOfmg override on an engine double whose cirsradg_ck_occultation is the un-collapsed restatement over the
double's cirsradg_ck_transmission."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occultation_cases as oc  # noqa: E402
import transit_cases as tc  # noqa: E402

REF = "/root/reference"
needs_reference = [pytest.mark.needs_reference,
                   pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "archnemesis")), reason="reference tree not present")]
TANHE = np.array([[40.0], [80.0], [130.0]])


def _mark(fn):
    for m in needs_reference:
        fn = m(fn)
    return fn


def test_restatement_reproduces_the_reference_occultation_and_gradients(oracle, golden_dir):
    """On the reference's own TAUTOT / dTAUTOT of the cut C1 case: SPECMOD rtol 1e-13, every non-zero column of dSPECMOD within
    1e-13 of its largest element, the 18 columns the reference leaves zero exactly zero.  Measured: SPECMOD 1.1e-16 absolute;
    columns 5.7e-16 at worst (tau_path stays below 4 on these six paths, so the merged down and up leg of Sm cost nothing)."""
    z = np.load(os.path.join(golden_dir, "occultation_c1.npz"))
    L = z["LAY_PRESS"].size
    NVMR, NDUST, NPRO = int(z["NVMR"]), int(z["NDUST"]), int(z["NPRO"])
    assert list(z["NLAYIN"]) == [110, 108, 94, 92, 78, 76] and L == 71 and z["LAYINC"].shape[0] == 110
    tan = oc.tangent_heights_km(z["BASEH"], z["NLAYIN"], z["LAYINC"])
    C = oc.tangent_mix(tan, z["TANHE"])
    Q = C.shape[0]
    assert C.shape == (3, 6) and np.all((C != 0).sum(axis=1) == 2) and np.allclose(C.sum(axis=1), 1.0)
    assert np.allclose(C @ tan, z["TANHE"][:, 0])                              # the interpolation puts each row at its tangent height
    Sm = tc.path_matrix(L, z["NLAYIN"], z["LAYINC"], z["SCALE"])
    MOD, TRANS, dMOD = oc.collapsed(z["TAUTOT"], np.asarray(z["DELG"], dtype=np.float64), Sm, C, z["dTAUTOT"], z["XFAC"])
    np.testing.assert_allclose(TRANS * z["XFAC"][:, None], z["SPECOUT"], rtol=1e-13)
    np.testing.assert_allclose(MOD, z["SPECMOD"], rtol=1e-13)
    W, NX = MOD.shape[0], z["xmap"].shape[0]
    pro = oracle.map2pro(dMOD, W, NVMR, NDUST, NPRO, Q, np.array([L] * Q), np.tile(np.arange(L)[:, None], (1, Q)), z["DTE"], z["DAM"],
                         z["DCO"], INCPAR=list(z["incpar"]))
    dspec = oracle.map2xvec(pro, W, NVMR, NDUST, NPRO, Q, NX, z["xmap"])
    ref = z["dSPECMOD"]
    scale = np.abs(ref).max(axis=(0, 1))
    assert np.count_nonzero(scale) == 63 and NX == 81
    err = np.abs(dspec - ref).max(axis=(0, 1)) / np.where(scale > 0, scale, 1.0)
    print("worst column %.3e (fixture: %.3e)" % (err.max(), z["restatement_err"].max()))
    assert err.max() <= 1e-13
    assert np.all(dspec[:, :, scale == 0] == 0.0)
    assert z["restatement_err"].shape == (NX,) and z["restatement_err"].max() <= 1e-13      # what the GPU test scales its bound by
    assert 0.018 < z["SPECONV"].min() < 0.02 and 0.89 < z["SPECONV"].max() < 0.9      # a real transmission spectrum
    assert np.count_nonzero(np.abs(z["dSPECONV"]).max(axis=(0, 1))) == 63


def _random_case(rng, W, G, L, NPAR, NLAYIN, LAYINC):
    LIMAX, P = LAYINC.shape
    tautot = 10.0 ** rng.uniform(-3, -1, (W, G, L))
    dtau = rng.uniform(-1, 1, (W, G, NPAR, L)) * 10.0 ** rng.uniform(-3, 0, (1, 1, NPAR, 1))
    SCALE = np.where(np.arange(LIMAX)[:, None] < NLAYIN[None, :], rng.uniform(1.0, 30.0, (LIMAX, P)), 0.0)
    delg = rng.uniform(0.5, 1.5, G); delg /= delg.sum()
    xfac = rng.uniform(0.5, 2.0, W)
    return tautot, dtau, SCALE, delg, xfac


def _assert_same(tautot, dtau, SCALE, delg, xfac, C, NLAYIN, LAYINC, L):
    """The two forms order their sums differently.  A path has at most 2 L = 24 entries here and tau_path < 24 x 30 x 0.1 = 72,
    so the rounding of tau_path reaches exp(-tau_path) as at most 72 x 24 x 2^-53 = 2e-13 relative; the sums over paths and g
    that follow add a few 2^-53 each.  1e-12 of the parameter slab's largest element is asked (of sum |C| for MOD)."""
    spec, dspec = tc.uncollapsed(tautot, delg, NLAYIN, LAYINC, SCALE, dtau)
    spec, dspec = spec * xfac[:, None], dspec * xfac[:, None, None, None]
    M0, dM0 = oc.mod_from_paths(spec, dspec, C, NLAYIN, LAYINC, L)
    M1, T1, dM1 = oc.collapsed(tautot, delg, tc.path_matrix(L, NLAYIN, LAYINC, SCALE), C, dtau, xfac)
    np.testing.assert_allclose(T1 * xfac[:, None], spec, rtol=1e-12)
    assert np.all(np.abs(M1 - M0) <= 1e-12 * xfac.max() * np.abs(C).sum(axis=1)[None, :])
    scale = np.abs(dM0).max(axis=(0, 2, 3), keepdims=True)
    assert np.max(np.abs(dM1 - dM0) / np.where(scale > 0, scale, 1.0)) < 1e-12
    return M1, dM1


def test_collapsed_form_equals_the_uncollapsed_form_on_ragged_paths():
    rng = np.random.default_rng(6)
    W, G, L, NPAR = 7, 4, 12, 5
    # bracketing pairs of limb paths as calc_pathg_SO makes them
    NLAYIN, LAYINC, _, bottoms = oc.occultation_paths(L, 3, rng)
    assert NLAYIN.size == 6 and np.array_equal(bottoms[1::2], bottoms[0::2] + 1) and np.array_equal(NLAYIN, 2 * (L - bottoms))
    C = np.zeros((3, 6))
    for q in range(3):
        C[q, 2 * q:2 * q + 2] = [0.3 + 0.1 * q, 0.7 - 0.1 * q]
    _, dM = _assert_same(*_random_case(rng, W, G, L, NPAR, NLAYIN, LAYINC), C, NLAYIN, LAYINC, L)
    assert np.abs(dM).max() > 0
    for q in range(3):                                   # below the lower path of its pair a geometry sees nothing
        assert np.all(dM[:, :, :bottoms[2 * q], q] == 0.0) and np.all(np.abs(dM[:, :, bottoms[2 * q]:, q]).max(axis=(0, 1)) > 0)
    # ragged: a path of two entries in one layer, a path that visits layers out of order and one twice, padding entries that
    # are 0 (not layer 0: layer 0 lies on the third path only), an empty path; a dense row, a row with a negative entry, an
    # empty row, a row on the empty path only
    LAYINC = np.zeros((6, 4), dtype=np.int32)
    NLAYIN = np.array([2, 5, 6, 0], dtype=np.int32)
    LAYINC[:2, 0] = [7, 7]
    LAYINC[:5, 1] = [11, 3, 9, 3, 5]
    LAYINC[:6, 2] = [4, 2, 0, 0, 2, 4]
    C = np.array([[0.5, 0.25, 1.5, 2.0], [1.0, -0.5, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 3.0]])
    case = _random_case(rng, W, G, L, NPAR, NLAYIN, LAYINC)
    M, dM = _assert_same(*case, C, NLAYIN, LAYINC, L)
    touched = np.zeros(L, bool); touched[[7, 11, 3, 9, 5, 4, 2, 0]] = True
    assert np.all(dM[:, :, ~touched, :] == 0.0) and np.all(np.abs(dM[:, :, touched, 0]).max(axis=(0, 1)) > 0)
    assert np.all(M[:, 2] == 0.0) and np.all(dM[..., 2] == 0.0)
    assert np.array_equal(M[:, 3], case[4] * 3.0) and np.all(dM[..., 3] == 0.0)       # the empty path: T = 1, no layer
    assert np.all(dM[:, :, [4, 2, 0], 1] == 0.0)                                       # row 1 does not name the third path


def test_tangent_mix_matches_the_restatement():
    """occultation.tangent_mix against the reference's loop restated: between two paths, below the lowest path (the lower
    neighbour -1 is the LAST path, as the Python index is), above the top path (weight 1 on it), exactly on a path, nearest path
    above the tangent height"""
    from archnemesis_dist_amd import occultation
    B = np.array([38.07, 42.68, 76.56, 82.07, 124.42, 130.94])
    T = np.array([[40.0], [80.0], [130.0], [20.0], [140.0], [76.56], [42.0], [130.94]])
    C = occultation.tangent_mix(B, T)
    R = oc.tangent_mix(B, T)
    assert C.shape == (8, 6) and np.array_equal(C, R)
    assert np.array_equal(C != 0, R != 0)
    np.testing.assert_allclose(C[0, :2], [1 - (40.0 - 38.07) / (42.68 - 38.07), 1 - (42.68 - 40.0) / (42.68 - 38.07)], rtol=1e-15)
    assert np.count_nonzero(C[0]) == 2 and np.count_nonzero(C[2]) == 2 and C[2, 4] > 0 and C[2, 5] > C[2, 4]
    # below the lowest path: paths 5 (wrapped) and 0, weights 1 - (20 - B5) / (B0 - B5) and 1 - (B0 - 20) / (B0 - B5)
    assert np.count_nonzero(C[3]) == 2
    np.testing.assert_allclose(C[3, [5, 0]], [1 - (20.0 - B[5]) / (B[0] - B[5]), 1 - (B[0] - 20.0) / (B[0] - B[5])], rtol=1e-15)
    assert np.array_equal(C[4], [0, 0, 0, 0, 0, 1.0])                                  # above the top path
    assert np.array_equal(C[5], [0, 0, 1.0, 0, 0, 0])                                  # on a path: fhl = 0, fhh = 1
    assert C[6, 0] > 0 and C[6, 1] > C[6, 0] and np.count_nonzero(C[6]) == 2           # nearest path above: its lower neighbour
    assert np.array_equal(C[7], [0, 0, 0, 0, 0, 1.0])                                  # on the top path
    assert np.array_equal(occultation.tangent_mix(B, T[:, 0]), C)
    rng = np.random.default_rng(2)
    L = 9
    NLAYIN, LAYINC, _ = tc.limb_paths(L, rng)
    BASEH = np.cumsum(rng.uniform(5e3, 4e4, L))
    assert np.array_equal(occultation.tangent_heights_km(BASEH, NLAYIN, LAYINC), oc.tangent_heights_km(BASEH, NLAYIN, LAYINC))


# ---- the adapter on the real reference, engine double ------------------------------------------------------------------
@pytest.fixture()
def so_case(oracle, monkeypatch):
    """The cut C1 case as a solar occultation of three geometries in a scratch directory, the reference imported, the adapter's
    engine replaced by the oracle double with the fused call restated un-collapsed."""
    import shutil
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.ref_import import import_reference
    from oracle import gen_golden_jacobian as gj
    from test_dropin_reference import OracleEngineDouble
    import archnemesis_dist_amd.forward_model as fmod

    class OccultationEngineDouble(OracleEngineDouble):
        occ_calls = 0

        def cirsradg_ck_occultation(self, lp, lt, am, taucont, dtaucon, NVMR, NPAR, igas_map, NLAYIN, LAYINC, SCALE, mix, xfac=None,
                                    gradients_on_device=False, dtau_every_gas=None):
            spec, dspec = self.cirsradg_ck_transmission(lp, lt, am, taucont, dtaucon, NVMR, NPAR, igas_map, NLAYIN, LAYINC, SCALE,
                                                        xfac=xfac)
            MOD, dMOD = oc.mod_from_paths(spec, dspec, np.asarray(mix), NLAYIN, np.asarray(LAYINC), len(lp))
            self.occ_calls += 1
            self._dmod = dMOD
            return MOD, spec, (None if gradients_on_device else dMOD)

        def map2pro(self, dSPECIN, *a, to_host=True, **k):
            out = self.orc.map2pro(self._dmod if dSPECIN is None else dSPECIN, *a, **k)
            self._pro = out
            return out if to_host else None

        def map2xvec(self, dSPECIN, *a, **k):
            return self.orc.map2xvec(self._pro if dSPECIN is None else dSPECIN, *a, **k)

    ans = import_reference()
    work = tempfile.mkdtemp(prefix="ansfm_occultation_")
    gj.setup_c1(ans, work)
    cwd = os.getcwd()
    os.chdir(work)
    double = OccultationEngineDouble(oracle)
    monkeypatch.setattr(fmod, "get_engine", lambda device=0: double)
    fmod.set_strict(True)
    fmod.reset_summary()

    def make(cls=None):
        fm = gj.cut_case(ans, cls=cls, nkeep=10, free=(20, 45, 70))
        M = fm.Measurement                                # as tests/test_jacobian_dropin.py sets a limb case up
        n0, ng = 10, 3
        rep = lambda a: np.repeat(np.asarray(a)[:n0, 0:1], ng, axis=1)
        M.NGEOM = ng
        M.NCONV = np.array([n0] * ng, dtype="int32")
        M.NAV = np.ones(ng, dtype="int32")
        M.VCONV = rep(M.VCONV); M.MEAS = rep(M.MEAS); M.ERRMEAS = rep(M.ERRMEAS)
        z = np.zeros((ng, 1))
        M.FLAT, M.FLON, M.AZI_ANG = z.copy(), z.copy(), z.copy()
        M.SOL_ANG = np.full((ng, 1), 60.0)
        M.EMISS_ANG = np.full((ng, 1), -1.0)
        M.TANHE = TANHE.copy()
        M.WGEOM = np.ones((ng, 1))
        M.NY = n0 * ng
        return fm

    try:
        yield ans, fmod, double, make
    finally:
        fmod.set_strict(False)
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)


def _quiet(fn, *a, **k):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _columns_agree(dspec, ref, tol):
    scale = np.abs(ref).max(axis=(0, 1))
    assert np.count_nonzero(scale) == 63
    err = np.abs(dspec - ref).max(axis=(0, 1)) / np.where(scale > 0, scale, 1.0)
    assert np.max(err[scale > 0]) <= tol
    assert np.all(dspec[:, :, scale == 0] == 0.0)


@_mark
def test_override_matches_the_reference_nemesisSOfmg(so_case):
    """(SPECONV, dSPECONV) of the override against the reference's own nemesisSOfmg(): SPECONV rtol 2e-7 (float32 table grids,
    as in test_jacobian_dropin.py), every non-zero column within 1e-8 of its largest element; the same through
    jacobian_nemesis(nemesisSO=True, analytical_gradient=True); exactly one fused call, the route counted, nothing delegated
    under set_strict(True)."""
    ans, fmod, double, make = so_case
    ref_spec, ref_dspec = _quiet(make().nemesisSOfmg)
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    spec, dspec = _quiet(make(FMGPU).nemesisSOfmg)
    assert double.occ_calls == 1 and getattr(double, "trg_calls", 0) == 1
    assert spec.shape == ref_spec.shape and dspec.shape == ref_dspec.shape
    np.testing.assert_allclose(spec, ref_spec, rtol=2e-7)
    _columns_agree(dspec, ref_dspec, 1e-8)
    routes = fmod.summary()["routes"]
    assert sum(v for k, v in routes.items() if "nemesisSOfmg" in k) == 1 and fmod.summary()["delegated"] == {}
    fm = make(FMGPU)
    YN, KK = _quiet(fm.jacobian_nemesis, NCores=1, nemesisSO=True, analytical_gradient=True)
    assert double.occ_calls == 2
    nc = int(fm.Measurement.NCONV[0])
    assert np.array_equal(YN, np.concatenate([spec[:nc, i] for i in range(3)]))
    analytic = np.asarray(fm.Variables.NUM) == 0
    assert analytic.any()
    assert np.array_equal(KK[:, analytic], np.concatenate([dspec[:nc, i, :] for i in range(3)])[:, analytic])


@_mark
def test_override_hands_aotf_telluric_and_an_engine_without_the_call_to_the_reference_method(so_case, monkeypatch):
    ans, fmod, double, make = so_case
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    seen = []
    monkeypatch.setattr(ans.ForwardModel_0, "nemesisSOfmg", lambda self: seen.append(1) or "reference")
    fm = make(FMGPU)
    fm.Telluric = object()
    assert fm.nemesisSOfmg() == "reference" and seen == [1] and double.occ_calls == 0
    fm = make(FMGPU)
    fm.Measurement.NORDERS_AOTF = 2
    assert fm.nemesisSOfmg() == "reference" and seen == [1, 1] and double.occ_calls == 0
    # ... and so does an engine without the fused call
    fm = make(FMGPU)
    monkeypatch.delattr(type(double), "cirsradg_ck_occultation")
    assert fm.nemesisSOfmg() == "reference" and seen == [1, 1, 1]


@_mark
def test_override_falls_back_when_the_engine_answers_unsupported(so_case, monkeypatch):
    """An engine that refuses the fused call (more than 320 layers or paths, no room for dMOD: NotImplementedError) sends the
    forward model to the reference's method, whose CIRSrad(return_grad=True) runs on the same engine; the fallback is noted in
    summary(), not counted as the fused route, and gives the numbers of the un-collapsed route."""
    ans, fmod, double, make = so_case
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    fused = _quiet(make(FMGPU).nemesisSOfmg)
    fmod.reset_summary()
    refused = []

    def unsupported(self, *a, **k):
        refused.append(1)
        raise NotImplementedError("cirsradg_ck_occultation: ANSFM_ERR_UNSUPPORTED")

    monkeypatch.setattr(type(double), "cirsradg_ck_occultation", unsupported)
    before = getattr(double, "trg_calls", 0)
    with pytest.warns(RuntimeWarning, match="fused occultation call"):
        spec, dspec = make(FMGPU).nemesisSOfmg()
    assert refused == [1] and double.trg_calls == before + 1            # CIRSrad(return_grad=True) of the reference's method
    summ = fmod.summary()
    assert any("fused occultation call" in k for k in summ["notes"]) and not any("nemesisSOfmg" in k for k in summ["routes"])
    assert summ["delegated"] == {}
    # the same opacities and the same gradients either way; only the order of the linear sums over paths, layers and levels
    # differs (at most 110 x 2 terms a column): 1e-12 of a column's largest element
    np.testing.assert_allclose(spec, fused[0], rtol=1e-12)
    _columns_agree(dspec, fused[1], 1e-12)
