"""Primary-transit depth with gradients, without a GPU: the NumPy restatement (tests/transit_cases.py) against the reference's
own nemesisPTfm(gradients=True) in tests/golden/transit_c1.npz (tools/golden/gen_golden_transit.py), the collapsed form
against the un-collapsed one on ragged paths, and -- where the reference tree is present -- the adapter's nemesisPTfm override
on an engine double whose cirsradg_ck_transit is the un-collapsed restatement over the double's cirsradg_ck_transmission."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transit_cases as tc  # noqa: E402

REF = "/root/reference"
needs_reference = [pytest.mark.needs_reference,
                   pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "archnemesis")), reason="reference tree not present")]


def _mark(fn):
    for m in needs_reference:
        fn = m(fn)
    return fn


def test_restatement_reproduces_the_reference_transit_depth_and_gradients(oracle, golden_dir):
    """On the reference's own TAUTOT / dTAUTOT of the cut C1 case: depth rtol 1e-13, every column of dSPECMOD within 1e-13 of
    its largest element.  Measured: depth 0.0; columns 8.5e-14 at worst -- a column whose largest element is 8e-57, where
    tau_path = 130 turns the rounding of its sum (down and up leg merged in Sm) into 130 times that in exp(-tau_path); the
    columns above 1e-30 of the largest one agree to 1e-15."""
    z = np.load(os.path.join(golden_dir, "transit_c1.npz"))
    L = z["LAY_PRESS"].size
    NVMR, NDUST, NPRO = int(z["NVMR"]), int(z["NDUST"]), int(z["NPRO"])
    tan = tc.tangent_heights_km(z["BASEH"], z["NLAYIN"], z["LAYINC"])
    c = tc.path_weights(tan, float(z["RADIUS"]))
    Sm = tc.path_matrix(L, z["NLAYIN"], z["LAYINC"], z["SCALE"])
    AREA, TRANS, dAREA = tc.collapsed(z["TAUTOT"], np.asarray(z["DELG"], dtype=np.float64), Sm, c, z["dTAUTOT"])
    spec, fac = tc.depth(AREA, float(z["RADIUS"]), tan[0], float(z["RSTAR_KM"]))
    # the path transmissions: tau_path is a sum of LIMAX products either way, each form with its own rounding, at most
    # LIMAX 2^-53 tau_path each; exp() turns that into a relative error, and tau_path = |ln T| reaches 150 here
    T = z["SPECOUT"]
    seen = T > 1e-300                                       # below: exp() has run out of exponent in both
    assert np.all(TRANS[~seen] <= 1e-300)
    assert np.all(np.abs(TRANS - T)[seen] <= (T * (1.0 - np.log(np.where(seen, T, 1.0))))[seen] * z["LAYINC"].shape[0] * 2.0 ** -52)
    np.testing.assert_allclose(spec, z["SPECMOD"][:, 0], rtol=1e-13)
    W, NX = spec.size, z["xmap"].shape[0]
    pro = oracle.map2pro(dAREA[..., None], W, NVMR, NDUST, NPRO, 1, np.array([L]), np.arange(L)[:, None], z["DTE"], z["DAM"], z["DCO"],
                         INCPAR=list(z["incpar"]))
    dspec = oracle.map2xvec(pro, W, NVMR, NDUST, NPRO, 1, NX, z["xmap"])[:, 0, :] * fac
    ref = z["dSPECMOD"][:, 0, :]
    scale = np.abs(ref).max(axis=0)
    assert np.count_nonzero(scale) == NX
    err = np.abs(dspec - ref).max(axis=0) / scale
    print("worst column %.3e (fixture: %.3e)" % (err.max(), z["restatement_err"].max()))
    assert err.max() <= 1e-13
    assert z["restatement_err"].shape == (NX,) and z["restatement_err"].max() <= 1e-13      # what the GPU test scales its bound by


def _random_case(rng, W, G, L, NPAR, NLAYIN, LAYINC):
    LIMAX, P = LAYINC.shape
    tautot = 10.0 ** rng.uniform(-3, -1, (W, G, L))
    dtau = rng.uniform(-1, 1, (W, G, NPAR, L)) * 10.0 ** rng.uniform(-3, 0, (1, 1, NPAR, 1))
    SCALE = np.where(np.arange(LIMAX)[:, None] < NLAYIN[None, :], rng.uniform(1.0, 30.0, (LIMAX, P)), 0.0)
    delg = rng.uniform(0.5, 1.5, G); delg /= delg.sum()
    c = rng.uniform(1e9, 1e11, P)
    return tautot, dtau, SCALE, delg, c


def _assert_same(tautot, dtau, SCALE, delg, c, NLAYIN, LAYINC, L):
    """The two forms order their sums differently.  A path has at most 2 L = 24 entries here and tau_path < 24 x 30 x 0.1 = 72,
    so the rounding of tau_path reaches exp(-tau_path) as at most 72 x 24 x 2^-53 = 2e-13 relative; the sums over paths and g
    that follow add a few 2^-53 each.  1e-12 of the parameter slab's largest element is asked."""
    spec, dspec = tc.uncollapsed(tautot, delg, NLAYIN, LAYINC, SCALE, dtau)
    A0, dA0 = tc.area_from_paths(spec, dspec, c, NLAYIN, LAYINC, L)
    A1, T1, dA1 = tc.collapsed(tautot, delg, tc.path_matrix(L, NLAYIN, LAYINC, SCALE), c, dtau)
    np.testing.assert_allclose(T1, spec, rtol=1e-12)
    np.testing.assert_allclose(A1, A0, rtol=1e-12, atol=0)
    scale = np.abs(dA0).max(axis=(0, 2), keepdims=True)
    assert np.max(np.abs(dA1 - dA0) / np.where(scale > 0, scale, 1.0)) < 1e-12
    return A1, dA1


def test_collapsed_form_equals_the_uncollapsed_form_on_ragged_paths():
    rng = np.random.default_rng(5)
    W, G, L, NPAR = 7, 4, 12, 5
    # limb paths as calc_path_PT makes them
    NLAYIN, LAYINC, _ = tc.limb_paths(L, rng)
    _, dA = _assert_same(*_random_case(rng, W, G, L, NPAR, NLAYIN, LAYINC), NLAYIN, LAYINC, L)
    assert np.abs(dA).max() > 0
    # ragged: a path of two entries in one layer, a path that visits layers out of order and one twice, padding entries that
    # are 0 (not layer 0: layer 0 lies on the third path only), an empty path
    LAYINC = np.zeros((6, 4), dtype=np.int32)
    NLAYIN = np.array([2, 5, 6, 0], dtype=np.int32)
    LAYINC[:2, 0] = [7, 7]
    LAYINC[:5, 1] = [11, 3, 9, 3, 5]
    LAYINC[:6, 2] = [4, 2, 0, 0, 2, 4]
    case = _random_case(rng, W, G, L, NPAR, NLAYIN, LAYINC)
    _, dA = _assert_same(*case, NLAYIN, LAYINC, L)
    touched = np.zeros(L, bool); touched[[7, 11, 3, 9, 5, 4, 2, 0]] = True
    assert np.all(dA[:, :, ~touched] == 0.0) and np.all(np.abs(dA[:, :, touched]).max(axis=(0, 1)) > 0)
    Sm = tc.path_matrix(L, NLAYIN, LAYINC, case[2])
    assert Sm[0, 0] == 0.0 and Sm[0, 1] == 0.0 and Sm[0, 3] == 0.0 and Sm[0, 2] == case[2][2, 2] + case[2][3, 2]
    # P = 1: the trapezoid has no interval, every weight is 0, AREA and every gradient are 0
    NLAYIN1, LAYINC1 = NLAYIN[1:2], LAYINC[:, 1:2]
    t, d, SC, dg, _ = _random_case(rng, W, G, L, NPAR, NLAYIN1, LAYINC1)
    c1 = tc.path_weights(np.array([12.5]), 7.0e7)
    assert c1.shape == (1,) and c1[0] == 0.0
    A, dA = _assert_same(t, d, SC, dg, c1, NLAYIN1, LAYINC1, L)
    assert np.all(A == 0.0) and np.all(dA == 0.0)


def test_package_geometry_helpers_match_the_restatement():
    from archnemesis_dist_amd import transit
    rng = np.random.default_rng(2)
    L = 9
    NLAYIN, LAYINC, _ = tc.limb_paths(L, rng)
    BASEH = np.cumsum(rng.uniform(5e3, 4e4, L))
    tan = tc.tangent_heights_km(BASEH, NLAYIN, LAYINC)
    assert np.array_equal(transit.tangent_heights_km(BASEH, NLAYIN, LAYINC), tan) and np.array_equal(tan, BASEH[:L - 1] / 1.0e3)
    np.testing.assert_allclose(transit.path_weights(tan, 6.9e7), tc.path_weights(tan, 6.9e7), rtol=1e-14)
    assert transit.path_weights(tan[:1], 6.9e7)[0] == 0.0


# ---- the adapter on the real reference, engine double ------------------------------------------------------------------
@pytest.fixture()
def pt_case(oracle, monkeypatch):
    """The cut C1 case as a primary transit in a scratch directory, the reference imported, the adapter's engine replaced by
    the oracle double with the fused call restated un-collapsed."""
    import shutil
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.ref_import import import_reference
    from oracle import gen_golden_jacobian as gj
    from test_dropin_reference import OracleEngineDouble
    import archnemesis_dist_amd.forward_model as fmod

    class TransitEngineDouble(OracleEngineDouble):
        transit_calls = 0

        def cirsradg_ck_transit(self, lp, lt, am, taucont, dtaucon, NVMR, NPAR, igas_map, NLAYIN, LAYINC, SCALE, path_weight,
                                gradients_on_device=False, dtau_every_gas=None):
            spec, dspec = self.cirsradg_ck_transmission(lp, lt, am, taucont, dtaucon, NVMR, NPAR, igas_map, NLAYIN, LAYINC, SCALE)
            AREA, dAREA = tc.area_from_paths(spec, dspec, np.asarray(path_weight), NLAYIN, np.asarray(LAYINC), len(lp))
            self.transit_calls += 1
            self._darea = dAREA
            return AREA, spec, (None if gradients_on_device else dAREA)

        def map2pro(self, dSPECIN, *a, to_host=True, **k):
            out = self.orc.map2pro(self._darea[..., None] if dSPECIN is None else dSPECIN, *a, **k)
            self._pro = out
            return out if to_host else None

        def map2xvec(self, dSPECIN, *a, **k):
            return self.orc.map2xvec(self._pro if dSPECIN is None else dSPECIN, *a, **k)

    ans = import_reference()
    work = tempfile.mkdtemp(prefix="ansfm_transit_")
    gj.setup_c1(ans, work)
    cwd = os.getcwd()
    os.chdir(work)
    double = TransitEngineDouble(oracle)
    monkeypatch.setattr(fmod, "get_engine", lambda device=0: double)
    fmod.set_strict(True)
    fmod.reset_summary()

    def make(cls=None, iform=2):
        fm = gj.cut_case(ans, cls=cls, nkeep=10, free=(20, 45, 70))
        fm.Measurement.IFORM = iform
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


@_mark
def test_override_matches_the_reference_nemesisPTfm_with_gradients(pt_case):
    """(SPECONV, dSPECONV) of the override against the reference's own nemesisPTfm(gradients=True): depth rtol 2e-7 (float32
    table grids, as in test_jacobian_dropin.py), every column within 1e-8 of its largest element; the same through
    jacobian_nemesis(nemesisPT=True, analytical_gradient=True); the route is counted and nothing is delegated."""
    ans, fmod, double, make = pt_case
    ref_spec, ref_dspec = _quiet(make().nemesisPTfm, gradients=True)
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    spec, dspec = _quiet(make(FMGPU).nemesisPTfm, gradients=True)
    assert double.transit_calls == 1 and getattr(double, "trg_calls", 0) == 1
    assert spec.shape == ref_spec.shape and dspec.shape == ref_dspec.shape
    np.testing.assert_allclose(spec, ref_spec, rtol=2e-7)
    scale = np.abs(ref_dspec).max(axis=(0, 1))
    assert np.count_nonzero(scale) == scale.size
    assert np.max(np.abs(dspec - ref_dspec).max(axis=(0, 1)) / scale) <= 1e-8
    routes = fmod.summary()["routes"]
    assert sum(v for k, v in routes.items() if "nemesisPTfm" in k) == 1 and fmod.summary()["delegated"] == {}
    fm = make(FMGPU)
    YN, KK = _quiet(fm.jacobian_nemesis, NCores=1, nemesisPT=True, analytical_gradient=True)
    assert double.transit_calls == 2
    nc = int(fm.Measurement.NCONV[0])
    assert np.array_equal(YN, spec[:nc, 0])
    analytic = np.asarray(fm.Variables.NUM) == 0
    assert analytic.any() and np.array_equal(KK[:, analytic], dspec[:nc, 0, :][:, analytic])


@_mark
def test_override_leaves_the_call_without_gradients_to_the_reference_method(pt_case):
    ans, fmod, double, make = pt_case
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    a = _quiet(make(FMGPU).nemesisPTfm, gradients=False)
    b = _quiet(ans.ForwardModel_0.nemesisPTfm, make(FMGPU), False)           # the reference class's method on the same kind of object
    assert np.array_equal(a, b) and double.transit_calls == 0
    assert np.array_equal(a, _quiet(make(FMGPU).nemesisPTfm))


@_mark
def test_override_raises_the_reference_error_for_another_unit(pt_case):
    ans, fmod, double, make = pt_case
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    with pytest.raises(ValueError, match="TransitDepth"):
        _quiet(make(FMGPU, iform=0).nemesisPTfm, gradients=True)
    assert double.transit_calls == 0


@_mark
def test_override_hands_a_telluric_case_to_the_reference_method(pt_case, monkeypatch):
    ans, fmod, double, make = pt_case
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    seen = []
    monkeypatch.setattr(ans.ForwardModel_0, "nemesisPTfm", lambda self, gradients=False: seen.append(gradients) or "reference")
    fm = make(FMGPU)
    fm.Telluric = object()
    assert fm.nemesisPTfm(gradients=True) == "reference" and seen == [True] and double.transit_calls == 0
    # ... and so does an engine without the fused call
    fm = make(FMGPU)
    monkeypatch.delattr(type(double), "cirsradg_ck_transit")
    assert fm.nemesisPTfm(gradients=True) == "reference" and seen == [True, True]


@_mark
def test_override_falls_back_when_the_engine_answers_unsupported(pt_case, monkeypatch):
    """An engine that refuses the fused call (more than 320 layers or paths: NotImplementedError) sends the forward model to the
    reference's method, whose CIRSrad(return_grad=True) runs on the same engine; the fallback is noted in summary(), not counted
    as the fused route, and gives the numbers of the un-collapsed route."""
    ans, fmod, double, make = pt_case
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    fused = _quiet(make(FMGPU).nemesisPTfm, gradients=True)
    fmod.reset_summary()
    refused = []

    def unsupported(self, *a, **k):
        refused.append(1)
        raise NotImplementedError("cirsradg_ck_transit: ANSFM_ERR_UNSUPPORTED")

    monkeypatch.setattr(type(double), "cirsradg_ck_transit", unsupported)
    before = getattr(double, "trg_calls", 0)
    with pytest.warns(RuntimeWarning, match="fused transit call"):
        spec, dspec = make(FMGPU).nemesisPTfm(gradients=True)
    assert refused == [1] and double.trg_calls == before + 1            # CIRSrad(return_grad=True) of the reference's method
    summ = fmod.summary()
    assert any("fused transit call" in k for k in summ["notes"]) and not any("nemesisPTfm" in k for k in summ["routes"])
    assert summ["delegated"] == {}
    # the same opacities and the same gradients either way; only the order of the linear sums over paths, layers and levels
    # differs (at most 142 x 70 terms a column): 1e-12 of a column's largest element
    np.testing.assert_allclose(spec, fused[0], rtol=1e-12)
    scale = np.abs(fused[1]).max(axis=(0, 1))
    assert np.max(np.abs(dspec - fused[1]).max(axis=(0, 1)) / scale) <= 1e-12
