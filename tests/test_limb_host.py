"""Limb thermal emission with gradients, without a GPU: the NumPy restatement (tests/limb_cases.py) against the reference's own
nemesisLfmg in tests/golden/limb_c1.npz (tools/golden/gen_golden_limb.py), the collapsed form against the un-collapsed one on
ragged paths whose legs differ in SCALE and EMTEMP, limb.tangent_mix against the restatement, and -- where the reference tree is
present -- the adapter's nemesisLfmg override on an engine double whose cirsradg_ck_limb is the un-collapsed restatement over the
double's cirsradg_ck_thermal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limb_cases as lc  # noqa: E402
import occultation_cases as oc  # noqa: E402

REF = "/root/reference"
needs_reference = [pytest.mark.needs_reference,
                   pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "archnemesis")), reason="reference tree not present")]
TANHE = np.array([[40.0], [80.0], [130.0]])


def _mark(fn):
    for m in needs_reference:
        fn = m(fn)
    return fn


def test_abi_declares_the_limb_entries():
    from archnemesis_dist_amd import _lib
    import ctypes as C
    vp, ci = C.c_void_p, C.c_int
    assert _lib.PROTOTYPES["ansfm_cirsradg_ck_limb"] == (ci, [vp, ci, ci] + [vp] * 5 + [ci, ci, vp, ci, ci] + [vp] * 4 + [ci] + [vp] * 7)
    assert _lib.PROTOTYPES["ansfm_limb_last"] == (ci, [vp, vp])


def test_restatement_reproduces_the_reference_limb_emission_and_gradients(oracle, golden_dir):
    """On the reference's own TAUTOT / dTAUTOT of the cut C1 case, with the bounds test_occultation_host.py holds the same
    comparison to: SPECMOD rtol 1e-13, every non-zero column of dSPECMOD within 1e-13 of its largest element, the 18 columns the
    reference leaves zero exactly zero.  Measured: SPECMOD 2.2e-16 relative; columns 2.8e-15 at worst (the tail sum of A_j formed
    as spec - prefix; summed directly, the un-collapsed form gives the same 2.8e-15)."""
    z = np.load(os.path.join(golden_dir, "limb_c1.npz"))
    assert os.path.getsize(os.path.join(golden_dir, "limb_c1.npz")) <= os.path.getsize(os.path.join(golden_dir, "occultation_c1.npz"))
    L = z["LAY_PRESS"].size
    NVMR, NDUST, NPRO, ISPACE = int(z["NVMR"]), int(z["NDUST"]), int(z["NPRO"]), int(z["ISPACE"])
    assert list(z["NLAYIN"]) == [110, 108, 94, 92, 78, 76] and L == 71 and z["LAYINC"].shape[0] == 110 and ISPACE == 0
    assert np.all(z["IMOD"] == 64)                                             # thermal emission
    assert all(lc.is_limb_path(z["LAY_PRESS"], z["NLAYIN"], z["LAYINC"], p) for p in range(6))
    tan = lc.tangent_heights_km(z["BASEH"], z["NLAYIN"], z["LAYINC"])
    C = lc.tangent_mix(tan, z["TANHE"])
    Q = C.shape[0]
    assert C.shape == (3, 6) and np.all((C != 0).sum(axis=1) == 2) and np.allclose(C.sum(axis=1), 1.0)
    assert np.allclose(C @ tan, z["TANHE"][:, 0])                              # the interpolation puts each row at its tangent height
    delg = np.asarray(z["DELG"], dtype=np.float64)
    args = (z["TAUTOT"], delg, z["NLAYIN"], z["LAYINC"], z["SCALE"], z["EMTEMP"])
    MOD, SPEC, dMOD = lc.collapsed(*args, C, ISPACE, z["WAVE"], NVMR, z["dTAUTOT"], z["XFAC"])
    np.testing.assert_allclose(SPEC * z["XFAC"][:, None], z["SPECOUT"], rtol=1e-13)
    np.testing.assert_allclose(MOD, z["SPECMOD"], rtol=1e-13)
    spec_u, dspec_u = lc.uncollapsed(*args, ISPACE, z["WAVE"], NVMR, z["dTAUTOT"], z["XFAC"])
    np.testing.assert_allclose(spec_u, z["SPECOUT"], rtol=1e-13)
    W, NX = MOD.shape[0], z["xmap"].shape[0]
    nl, li = np.array([L] * Q), np.tile(np.arange(L)[:, None], (1, Q))
    ref = z["dSPECMOD"]
    scale = np.abs(ref).max(axis=(0, 1))
    assert np.count_nonzero(scale) == 63 and NX == 81
    for what, d in (("collapsed", dMOD), ("un-collapsed", oc.mod_from_paths(spec_u, dspec_u, C, z["NLAYIN"], z["LAYINC"], L)[1])):
        pro = oracle.map2pro(d, W, NVMR, NDUST, NPRO, Q, nl, li, z["DTE"], z["DAM"], z["DCO"], INCPAR=list(z["incpar"]))
        dspec = oracle.map2xvec(pro, W, NVMR, NDUST, NPRO, Q, NX, z["xmap"])
        err = np.abs(dspec - ref).max(axis=(0, 1)) / np.where(scale > 0, scale, 1.0)
        print("%s: worst column %.3e (fixture: %.3e)" % (what, err.max(), z["restatement_err"].max()))
        assert err.max() <= 1e-13
        assert np.all(dspec[:, :, scale == 0] == 0.0)
    assert z["restatement_err"].shape == (NX,) and z["restatement_err"].max() <= 1e-13      # what the GPU test scales its bound by
    assert 5e-10 < z["SPECONV"].min() < 6e-10 and 4e-8 < z["SPECONV"].max() < 5e-8          # a real radiance spectrum
    assert np.count_nonzero(np.abs(z["dSPECONV"]).max(axis=(0, 1))) == 63


def _random_case(rng, W, G, L, NPAR, NLAYIN, LAYINC):
    LIMAX, P = LAYINC.shape
    inside = np.arange(LIMAX)[:, None] < NLAYIN[None, :]
    tautot = 10.0 ** rng.uniform(-3, -1, (W, G, L))
    dtau = rng.uniform(-1, 1, (W, G, NPAR, L)) * 10.0 ** rng.uniform(-3, 0, (1, 1, NPAR, 1))
    SCALE = np.where(inside, rng.uniform(1.0, 30.0, (LIMAX, P)), 0.0)
    EMTEMP = np.where(inside, rng.uniform(120.0, 260.0, (LIMAX, P)), 0.0)
    delg = rng.uniform(0.5, 1.5, G); delg /= delg.sum()
    xfac = rng.uniform(0.5, 2.0, W)
    return tautot, dtau, SCALE, EMTEMP, delg, xfac


def _assert_same(ispace, wave, NVMR, tautot, dtau, SCALE, EMTEMP, delg, xfac, C, NLAYIN, LAYINC, L):
    """The two forms order their sums differently, and the collapsed one forms the tail sum of A_j as spec - prefix.  A path has
    at most 2 L = 24 entries here and tau_path < 24 x 30 x 0.1 = 72, so the rounding of the running product T_j is at most
    24 x 2 x 2^-53 = 5e-15 relative; spec - prefix is off by at most 24 x 2^-53 spec = 3e-15 spec, which A_j = T_j B_j - tail
    carries absolutely while |A_j| reaches max_j B_j >= spec somewhere on the path; the sums over entries, paths and g add a few
    2^-53 each.  1e-12 of the parameter slab's largest element is asked (of sum |C| max SPEC for MOD)."""
    spec, dspec = lc.uncollapsed(tautot, delg, NLAYIN, LAYINC, SCALE, EMTEMP, ispace, wave, NVMR, dtau, xfac)
    M0, dM0 = oc.mod_from_paths(spec, dspec, C, NLAYIN, LAYINC, L)
    M1, S1, dM1 = lc.collapsed(tautot, delg, NLAYIN, LAYINC, SCALE, EMTEMP, C, ispace, wave, NVMR, dtau, xfac)
    np.testing.assert_allclose(S1 * xfac[:, None], spec, rtol=1e-12)
    assert np.all(np.abs(M1 - M0) <= 1e-12 * xfac.max() * np.abs(C).sum(axis=1)[None, :] * S1.max())
    scale = np.abs(dM0).max(axis=(0, 2, 3), keepdims=True)
    assert np.all(scale > 0)
    assert np.max(np.abs(dM1 - dM0) / scale) < 1e-12
    return M1, dM1


@pytest.mark.parametrize("ispace", [0, 1])
def test_collapsed_form_equals_the_uncollapsed_form_on_ragged_paths(ispace):
    rng = np.random.default_rng(6 + ispace)
    W, G, L, NPAR, NVMR = 7, 4, 12, 5, 3
    wave = np.linspace(600.0, 900.0, W) if ispace == 0 else np.linspace(8.0, 14.0, W)
    # bracketing pairs of limb paths as calc_pathg_L makes them; the two legs of a path differ in SCALE and EMTEMP
    NLAYIN, LAYINC, _, _, bottoms = lc.limb_pairs(L, 3, rng)
    assert NLAYIN.size == 6 and np.array_equal(bottoms[1::2], bottoms[0::2] + 1) and np.array_equal(NLAYIN, 2 * (L - bottoms))
    C = np.zeros((3, 6))
    for q in range(3):
        C[q, 2 * q:2 * q + 2] = [0.3 + 0.1 * q, 0.7 - 0.1 * q]
    case = _random_case(rng, W, G, L, NPAR, NLAYIN, LAYINC)
    n0 = int(NLAYIN[0])
    assert not np.array_equal(case[2][:n0 // 2, 0], case[2][n0 - 1:n0 // 2 - 1:-1, 0])       # SCALE: down leg != up leg
    assert not np.array_equal(case[3][:n0 // 2, 0], case[3][n0 - 1:n0 // 2 - 1:-1, 0])       # EMTEMP likewise
    _, dM = _assert_same(ispace, wave, NVMR, *case, C, NLAYIN, LAYINC, L)
    for q in range(3):                                   # below the lower path of its pair a geometry sees nothing
        assert np.all(dM[:, :, :bottoms[2 * q], q] == 0.0) and np.all(np.abs(dM[:, :, bottoms[2 * q]:, q]).max(axis=(0, 1)) > 0)
    # two adjacent geometries that share a path (ITANHE of calc_pathg_L is np.unique'd): 4 paths for 3 geometries
    keep = np.array([0, 1, 3, 5])
    C = np.array([[0.4, 0.6, 0.0, 0.0], [0.0, 0.25, 0.75, 0.0], [0.0, 0.0, 0.1, 0.9]])
    _assert_same(ispace, wave, NVMR, case[0], case[1], case[2][:, keep], case[3][:, keep], case[4], case[5], C, NLAYIN[keep],
                 LAYINC[:, keep], L)
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
    M, dM = _assert_same(ispace, wave, NVMR, *case, C, NLAYIN, LAYINC, L)
    touched = np.zeros(L, bool); touched[[7, 11, 3, 9, 5, 4, 2, 0]] = True
    assert np.all(dM[:, :, ~touched, :] == 0.0) and np.all(np.abs(dM[:, :, touched, 0]).max(axis=(0, 1)) > 0)
    assert np.all(M[:, 2] == 0.0) and np.all(dM[..., 2] == 0.0)
    assert np.all(M[:, 3] == 0.0) and np.all(dM[..., 3] == 0.0)                        # the empty path emits nothing
    assert np.all(dM[:, :, [4, 2, 0], 1] == 0.0)                                       # row 1 does not name the third path


def test_limb_geometry_is_the_occultation_geometry():
    """:1444-1446 and :1475-1496 are :1180-1182 and :1211-1232 line for line, so limb.py re-exports; the restated loop agrees"""
    from archnemesis_dist_amd import limb, occultation
    assert limb.tangent_mix is occultation.tangent_mix and limb.tangent_heights_km is occultation.tangent_heights_km
    B = np.array([38.07, 42.68, 76.56, 82.07, 124.42, 130.94])
    T = np.array([[40.0], [80.0], [130.0], [20.0], [140.0], [76.56], [42.0], [130.94]])
    assert np.array_equal(limb.tangent_mix(B, T), lc.tangent_mix(B, T))
    # adjacent tangent heights inside one bracket, as calc_pathg_L leaves them after np.unique: both rows on the same two paths
    C = limb.tangent_mix(B, np.array([39.0, 41.0]))
    assert np.array_equal(C != 0, [[True, True, False, False, False, False]] * 2)


# ---- the adapter on the real reference, engine double ------------------------------------------------------------------
@pytest.fixture()
def limb_case(oracle, monkeypatch):
    """The cut C1 case as a limb observation of three geometries in a scratch directory, the reference imported, the adapter's
    engine replaced by the oracle double with the fused call restated un-collapsed."""
    import shutil
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.ref_import import import_reference
    from oracle import gen_golden_jacobian as gj
    from test_dropin_reference import OracleEngineDouble
    import archnemesis_dist_amd.forward_model as fmod

    class LimbEngineDouble(OracleEngineDouble):
        limb_calls = 0
        thg_calls = 0

        def cirsradg_ck_thermal(self, *a, **k):
            self.thg_calls += 1
            return super().cirsradg_ck_thermal(*a, **k)

        def cirsradg_ck_limb(self, ISPACE, lp, lt, am, taucont, dtaucon, NVMR, NPAR, igas_map, NLAYIN, LAYINC, SCALE, EMTEMP, mix,
                             xfac=None, gradients_on_device=False, dtau_every_gas=None):
            if not all(lc.is_limb_path(np.asarray(lp), NLAYIN, np.asarray(LAYINC), p) for p in range(len(NLAYIN))):
                raise NotImplementedError("cirsradg_ck_limb: a path ends at the lower boundary")      # as the engine answers
            spec, dspec, _ = OracleEngineDouble.cirsradg_ck_thermal(self, ISPACE, lp, lt, am, taucont, dtaucon, NVMR, NPAR, igas_map,
                                                                    NLAYIN, LAYINC, SCALE, EMTEMP, -1.0, xfac=xfac)
            MOD, dMOD = oc.mod_from_paths(spec, dspec, np.asarray(mix), NLAYIN, np.asarray(LAYINC), len(lp))
            self.limb_calls += 1
            self._dmod = dMOD
            return MOD, spec, (None if gradients_on_device else dMOD)

        def map2pro(self, dSPECIN, *a, to_host=True, **k):
            out = self.orc.map2pro(self._dmod if dSPECIN is None else dSPECIN, *a, **k)
            self._pro = out
            return out if to_host else None

        def map2xvec(self, dSPECIN, *a, **k):
            return self.orc.map2xvec(self._pro if dSPECIN is None else dSPECIN, *a, **k)

    ans = import_reference()
    work = tempfile.mkdtemp(prefix="ansfm_limb_")
    gj.setup_c1(ans, work)
    cwd = os.getcwd()
    os.chdir(work)
    double = LimbEngineDouble(oracle)
    monkeypatch.setattr(fmod, "get_engine", lambda device=0: double)
    fmod.set_strict(True)
    fmod.reset_summary()

    def make(cls=None):
        fm = gj.cut_case(ans, cls=cls, nkeep=10, free=(20, 45, 70))
        M = fm.Measurement                                # as tools/golden/gen_golden_limb.py sets the case up
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
    print("columns by err:", np.array2string(err[scale > 0], precision=2))
    assert np.all(err[scale > 0] <= np.broadcast_to(tol, err.shape)[scale > 0])
    assert np.all(dspec[:, :, scale == 0] == 0.0)


@_mark
def test_override_reproduces_the_golden_nemesisLfmg(limb_case, golden_dir):
    """(SPECONV, dSPECONV) of the override against the reference's own nemesisLfmg() in the fixture: SPECONV rtol 2e-7 (float32
    table grids, as in test_jacobian_dropin.py); every non-zero column of dSPECONV within 1e-8 of its largest element, the bound
    test_occultation_host.py asks of the same comparison, plus the allowance derived in lc.cancellation_terms for the rounding of
    T_{j-1} - T_j: libm's exp and NumPy's may differ by an ulp, which with the product and the subtraction is up to 4 x 2^-53 T_{j-1}
    on a difference that is tau_j T_{j-1} ~ 1e-9 T_{j-1} in the thin top layers.  The allowance is formed on dSPECMOD and applied
    to dSPECONV (the convolution is a weighted mean over nine wavenumbers).  It is below 1e-8 for all but the last nine columns and
    3.8e-5 for the topmost temperature level (measured there: 8.3e-7; the other columns 1e-15 .. 1e-9; the Jacobian contract is
    1e-4).  The same through jacobian_nemesis(nemesisL=True, analytical_gradient=True); exactly one
    fused call each and no un-collapsed one, the route counted, nothing delegated under set_strict(True)."""
    ans, fmod, double, make = limb_case
    z = np.load(os.path.join(golden_dir, "limb_c1.npz"))
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    spec, dspec = _quiet(make(FMGPU).nemesisLfmg)
    assert double.limb_calls == 1 and double.thg_calls == 0
    assert spec.shape == z["SPECONV"].shape and dspec.shape == z["dSPECONV"].shape
    np.testing.assert_allclose(spec, z["SPECONV"], rtol=2e-7)
    allowance = 4.0 * 2.0 ** -53 * lc.golden_cancellation_by_column(z, double.orc)
    assert np.count_nonzero(allowance > 1e-8) <= 9 and allowance.max() < 5e-5
    _columns_agree(dspec, z["dSPECONV"], 1e-8 + allowance)
    routes = fmod.summary()["routes"]
    assert sum(v for k, v in routes.items() if "nemesisLfmg" in k) == 1 and fmod.summary()["delegated"] == {}
    fm = make(FMGPU)
    YN, KK = _quiet(fm.jacobian_nemesis, NCores=1, nemesisL=True, analytical_gradient=True)
    assert double.limb_calls == 2 and double.thg_calls == 0 and fmod.summary()["delegated"] == {}
    nc = int(fm.Measurement.NCONV[0])
    assert np.array_equal(YN, np.concatenate([spec[:nc, i] for i in range(3)]))
    analytic = np.asarray(fm.Variables.NUM) == 0
    assert analytic.any()
    assert np.array_equal(KK[:, analytic], np.concatenate([dspec[:nc, i, :] for i in range(3)])[:, analytic])
    np.testing.assert_allclose(YN, np.concatenate([z["SPECONV"][:nc, i] for i in range(3)]), rtol=2e-7)


@_mark
def test_override_hands_every_case_it_does_not_take_to_the_reference_method(limb_case, monkeypatch):
    """Telluric, runtime line-by-line, a case _ansfm_supported(True) declines, a path calculation that is not thermal emission,
    a path that ends at the lower boundary (the engine refuses it, as any case it does not take, and the fallback is noted) and
    an engine without the call: the reference's method, never an error, and no fused call."""
    ans, fmod, double, make = limb_case
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    seen = []
    monkeypatch.setattr(ans.ForwardModel_0, "nemesisLfmg", lambda self: seen.append(1) or "reference")
    fm = make(FMGPU)
    fm.Telluric = object()
    assert fm.nemesisLfmg() == "reference" and len(seen) == 1
    orig_paths = ans.ForwardModel_0.calc_pathg_L

    def after_paths(change):
        def calc_pathg_L(self, *a, **k):
            out = orig_paths(self, *a, **k)
            change(self)
            return out
        return calc_pathg_L

    def runtime_lbl(self):
        self.SpectroscopyX.ILBL = fmod.ILBL_LBL_RUNTIME          # no LINE_DATA: _ansfm_line_source declines

    def not_thermal(self):
        self.PathX.IMOD = np.zeros_like(np.asarray(self.PathX.IMOD))      # pure transmission

    def to_the_ground(self):
        self.LayerX.PRESS = np.ascontiguousarray(np.asarray(self.LayerX.PRESS)[::-1])      # the last layer now lies deepest

    for n, change in enumerate((runtime_lbl, not_thermal, to_the_ground), start=2):
        monkeypatch.setattr(ans.ForwardModel_0, "calc_pathg_L", after_paths(change))
        assert _quiet(make(FMGPU).nemesisLfmg) == "reference" and len(seen) == n, change.__name__
    monkeypatch.setattr(ans.ForwardModel_0, "calc_pathg_L", orig_paths)
    with monkeypatch.context() as m:
        m.setattr(fmod.CIRSradGPU, "_ansfm_supported", lambda self, return_grad: False)
        assert _quiet(make(FMGPU).nemesisLfmg) == "reference" and len(seen) == 5
    assert double.limb_calls == 0
    monkeypatch.delattr(type(double), "cirsradg_ck_limb")
    assert make(FMGPU).nemesisLfmg() == "reference" and len(seen) == 6


@_mark
def test_override_falls_back_when_the_engine_answers_unsupported(limb_case, monkeypatch):
    """An engine that refuses the fused call (more than 160 layers, a path to the ground, no room for dMOD or the scratch:
    NotImplementedError) sends the forward model to the reference's method, whose CIRSrad(return_grad=True) runs on the same
    engine; the fallback is noted in summary(), not counted as the fused route, and gives the numbers of the un-collapsed route."""
    ans, fmod, double, make = limb_case
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    fused = _quiet(make(FMGPU).nemesisLfmg)
    fmod.reset_summary()
    refused = []

    def unsupported(self, *a, **k):
        refused.append(1)
        raise NotImplementedError("cirsradg_ck_limb: ANSFM_ERR_UNSUPPORTED")

    monkeypatch.setattr(type(double), "cirsradg_ck_limb", unsupported)
    assert double.thg_calls == 0
    with pytest.warns(RuntimeWarning, match="fused limb call"):
        spec, dspec = make(FMGPU).nemesisLfmg()
    assert refused == [1] and double.thg_calls == 1                      # CIRSrad(return_grad=True) of the reference's method
    summ = fmod.summary()
    assert any("fused limb call" in k for k in summ["notes"]) and not any("nemesisLfmg" in k for k in summ["routes"])
    assert summ["delegated"] == {}
    # the same opacities and the same gradients either way; only the order of the linear sums over paths, layers and levels
    # differs (at most 110 x 2 terms a column): 1e-12 of a column's largest element
    np.testing.assert_allclose(spec, fused[0], rtol=1e-12)
    _columns_agree(dspec, fused[1], 1e-12)
