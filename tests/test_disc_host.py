"""Disc average with gradients, without a GPU: the NumPy restatement (tests/disc_cases.py) against the reference's own
nemesisdiscfmg in tests/golden/disc_c1.npz (tools/golden/gen_golden_disc.py), the collapsed form against the un-collapsed one on
ragged SCALE columns with and without the ground and on both TSURF branches, disc.average_mix / disc.shared_sequence, and --
where the reference tree is present -- the adapter's nemesisdiscfmg override on an engine double whose cirsradg_ck_disc is the
un-collapsed restatement over the double's cirsradg_ck_thermal."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import disc_cases as dc  # noqa: E402

REF = "/root/reference"
needs_reference = [pytest.mark.needs_reference,
                   pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "archnemesis")), reason="reference tree not present")]
EMISS_ANG = np.array([[0.0, 40.0, 65.0]])
WGEOM = np.array([[0.2, 0.5, 0.3]])


def _mark(fn):
    for m in needs_reference:
        fn = m(fn)
    return fn


def test_abi_declares_the_disc_entries():
    from archnemesis_dist_amd import _lib
    import ctypes as C
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    assert _lib.PROTOTYPES["ansfm_cirsradg_ck_disc"] == (
        ci, [vp, ci, ci] + [vp] * 5 + [ci, ci, vp, ci, vp, vp, ci, vp, cd, vp, ci] + [vp] * 8)
    assert _lib.PROTOTYPES["ansfm_disc_last"] == (ci, [vp, vp])
    header = open(os.path.join(_lib.INCLUDE, "ansfm.h")).read()
    assert "GS = min(G, max(4, ceil(256 / ((Wpad / 64) (Q + u)))))" in header          # the g-groups behind the scratch formula


@pytest.mark.parametrize("case", ["", "S_"])
def test_restatement_reproduces_the_reference_disc_average_and_gradients(oracle, golden_dir, case):
    """On the reference's own TAUTOT / dTAUTOT of the cut C1 case, without a surface and (S_) with one at 180 K: SPEC rtol 1e-13,
    every column of dSPEC within 1e-10 of its largest element (the project's column bound; measured 1.4e-15, the limb's was
    2.8e-15), sum WGEOM dTSURF likewise (measured 3e-17); the stored restatement errors are what is measured here."""
    path = os.path.join(golden_dir, "disc_c1.npz")
    z = np.load(path)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(golden_dir, "limb_c1.npz"))
    g = lambda k: z[case + k] if case + k in z.files else z[k]
    L = z["LAY_PRESS"].size
    NVMR, NDUST, NPRO = int(z["NVMR"]), int(z["NDUST"]), int(z["NPRO"])
    assert z["LAYINC"].size == 71 and L == 71 and list(z["LAYINC"][[0, -1]]) == [70, 0] and int(z["ISPACE"]) == 0
    assert np.all(z["IMOD"] == 64) and dc.is_ground(z["LAY_PRESS"], z["LAYINC"])
    assert z["SCALE"].shape == (71, 3) and np.allclose(z["SCALE"][0], [1.0, 1.2994, 2.2974], atol=1e-4)
    assert bool(z["fmg_equals_discfmg"])                      # nemesisfmg()'s NAV > 1 loop is the same algebra, bit for bit
    assert float(z["TSURF"]) == 0.0 and float(z["S_TSURF"]) == 180.0 and np.ptp(z["S_EMISSIVITY"]) > 0.1
    args, kw = dc.golden_inputs(z, case)
    MOD, SPEC, dTSMOD, dMOD = dc.collapsed(*args, **kw)
    np.testing.assert_allclose(SPEC * z["XFAC"][:, None], g("SPECOUT"), rtol=1e-13)
    np.testing.assert_allclose(MOD[:, 0], g("SPEC"), rtol=1e-13)
    su, dsu, dtu = dc.uncollapsed(*args[:8], *args[9:], **kw)
    np.testing.assert_allclose(su, g("SPECOUT"), rtol=1e-13)
    np.testing.assert_allclose(dtu, g("dTSURF"), rtol=1e-13)
    W, NX = MOD.shape[0], z["xmap"].shape[0]
    ref = g("dSPEC")
    scale = np.abs(ref).max(axis=0)
    assert np.count_nonzero(scale) == NX == 81
    C = args[8]
    for what, (d, ts) in (("collapsed", (dMOD, dTSMOD)), ("un-collapsed", dc.mod_from_points(su, dsu, dtu, C, z["LAYINC"], L)[:0:-1])):
        pro = oracle.map2pro(d, W, NVMR, NDUST, NPRO, 1, np.array([L]), np.arange(L)[:, None], z["DTE"], z["DAM"], z["DCO"],
                             INCPAR=list(z["incpar"]))
        dspec = oracle.map2xvec(pro, W, NVMR, NDUST, NPRO, 1, NX, z["xmap"])[:, 0, :]
        err = np.abs(dspec - ref).max(axis=0) / scale
        ts_ref = g("dTSURF") @ WGEOM[0]
        ts_err = np.abs(ts[:, 0] - ts_ref).max() / np.abs(ts_ref).max()
        print("%s: worst column %.3e (fixture: %.3e); sum WGEOM dTSURF %.3e" % (what, err.max(), g("restatement_err").max(), ts_err))
        assert np.all(err <= 1e-10) and ts_err <= 1e-10
    assert g("restatement_err").shape == (NX,) and np.all(g("restatement_err") <= 1e-10) and float(g("restatement_err_dtsurf")) <= 1e-10
    assert 3e-9 < z["SPECONV"].min() and z["SPECONV"].max() < 6e-8                          # a real radiance spectrum
    assert np.abs(g("SPEC") - z["SPEC"]).max() > 0 if case else True                        # the surface changes the spectrum


def _random_case(rng, W, G, L, NPAR, N, P):
    tautot = 10.0 ** rng.uniform(-3, -1, (W, G, L))
    dtau = rng.uniform(-1, 1, (W, G, NPAR, L)) * 10.0 ** rng.uniform(-3, 0, (1, 1, NPAR, 1))
    SCALE = rng.uniform(1.0, 30.0, (N, P))                     # ragged columns: no path a multiple of another
    EMTEMP = rng.uniform(120.0, 260.0, N)
    delg = rng.uniform(0.5, 1.5, G); delg /= delg.sum()
    xfac = rng.uniform(0.5, 2.0, W)
    return tautot, dtau, SCALE, EMTEMP, delg, xfac


@pytest.mark.parametrize("ispace", [0, 1])
@pytest.mark.parametrize("tsurf", [-1.0, 180.0])
@pytest.mark.parametrize("ground", [True, False])
def test_collapsed_form_equals_the_uncollapsed_form_on_ragged_scale_columns(ispace, tsurf, ground):
    """The two forms order their sums differently, and the collapsed one forms the tail sum of A_j as spec_atm - prefix with the
    ground's term apart.  A sequence has at most 2 L = 24 entries and tau_path < 24 x 30 x 0.1 = 72, so the bounds test_limb_host.py
    derives for the same comparison hold: the running product is off by at most 24 x 2 x 2^-53 = 5e-15 relative, spec - prefix by
    3e-15 spec; the ground adds T_end R <= max(B, R) with the product's error.  1e-12 of the parameter slab's largest element is
    asked (of sum |C| max SPEC for MOD, of sum |C| max dTSURF for dTSMOD)."""
    rng = np.random.default_rng(16 + ispace + 2 * ground + 4 * (tsurf > 0))
    W, G, L, NPAR, NVMR, P = 7, 4, 12, 5, 3, 4
    wave = np.linspace(600.0, 900.0, W) if ispace == 0 else np.linspace(8.0, 14.0, W)
    lay_press = np.logspace(4.5, 0.5, L)                       # layer 0 the deepest
    if ground:
        LAYINC = np.arange(L - 1, -1, -1)
    else:                                                      # down to layer 2 and up again, layer 5 skipped on the way up
        LAYINC = np.concatenate([np.arange(L - 1, 1, -1), [2, 3, 4, 6, 7, 8, 9, 10, 11]])
    N = LAYINC.size
    assert dc.is_ground(lay_press, LAYINC) == ground
    tautot, dtau, SCALE, EMTEMP, delg, xfac = _random_case(rng, W, G, L, NPAR, N, P)
    emis = rng.uniform(0.5, 1.0, W) if tsurf > 0 else None
    C = np.array([[0.2, 0.5, 0.3, 0.0], [0.0, -0.5, 1.5, 0.0], [0.0, 0.0, 0.0, 0.0]])       # a shared path, an orphan, an empty row
    seq = (tautot, delg, lay_press, LAYINC, SCALE, EMTEMP, tsurf, emis)
    spec, dspec, dts = dc.uncollapsed(*seq, ispace, wave, NVMR, dtau, xfac)
    M0, T0, dM0 = dc.mod_from_points(spec, dspec, dts, C, LAYINC, L)
    M1, S1, T1, dM1 = dc.collapsed(*seq, C, ispace, wave, NVMR, dtau, xfac)
    np.testing.assert_allclose(S1 * xfac[:, None], spec, rtol=1e-12)
    Cs = np.abs(C).sum(axis=1)[None, :]
    assert np.all(np.abs(M1 - M0) <= 1e-12 * xfac.max() * Cs * S1.max())
    assert np.all(np.abs(T1 - T0) <= 1e-12 * Cs * np.abs(dts).max())
    scale = np.abs(dM0).max(axis=(0, 2, 3), keepdims=True)
    assert np.all(scale > 0) and np.max(np.abs(dM1 - dM0) / scale) < 1e-12
    assert np.all(M1[:, 2] == 0.0) and np.all(T1[:, 2] == 0.0) and np.all(dM1[..., 2] == 0.0)
    if ground:
        assert np.all(np.abs(T1[:, :2]) > 0)
        # the reference's quirk: with TSURF <= 0 the ground still has a dTSURF, T_end dB/dT at the last entry's temperature
        if tsurf <= 0:
            T_end = np.exp(-np.einsum("wgj,j->wg", tautot[:, :, LAYINC], SCALE[:, 0]))
            np.testing.assert_allclose(dts[:, 0], xfac * (T_end @ delg) * dc.planckg(ispace, wave, EMTEMP[-1])[1], rtol=1e-12)
    else:
        assert np.all(T1 == 0.0) and np.all(dts == 0.0)
        untouched = np.setdiff1d(np.arange(L), LAYINC)
        assert list(untouched) == [0, 1] and np.all(dM1[:, :, untouched, :] == 0.0)


def _point(press, temp, scale, tsurf=0.0, npath=1):
    n = len(scale)
    layer = SimpleNamespace(PRESS=press, TEMP=temp, AMOUNT=np.outer(press, [1.0, 2.0]), DTE=np.ones((len(press), 3)),
                            DAM=np.ones((len(press), 3)), DCO=np.ones((len(press), 3)))
    path = SimpleNamespace(NPATH=npath, NLAYIN=np.array([n] * npath), LAYINC=np.tile(np.arange(n - 1, -1, -1)[:, None], (1, npath)),
                           EMTEMP=np.tile(temp[::-1][:, None], (1, npath)), SCALE=np.tile(np.asarray(scale)[:, None], (1, npath)))
    return layer, path, SimpleNamespace(TSURF=tsurf), np.ones((2, 4, 3))


def test_average_mix_and_shared_sequence():
    from archnemesis_dist_amd import disc
    C = disc.average_mix(WGEOM[0])
    assert C.shape == (1, 3) and C.dtype == np.float64 and np.array_equal(C[0], [0.2, 0.5, 0.3]) and C.flags.c_contiguous
    press, temp = np.logspace(5, 1, 6), np.linspace(200.0, 120.0, 6)
    scales = [np.full(6, 1.0), np.full(6, 1.2994), np.linspace(2.0, 2.5, 6)]
    points = [_point(press.copy(), temp.copy(), s) for s in scales]
    LAYINC, EMTEMP, SCALE = disc.shared_sequence(points)
    assert LAYINC.dtype == np.int32 and list(LAYINC) == [5, 4, 3, 2, 1, 0] and np.array_equal(EMTEMP, temp[::-1])
    assert SCALE.shape == (6, 3) and all(np.array_equal(SCALE[:, i], scales[i]) for i in range(3)) and SCALE.flags.c_contiguous
    assert disc.shared_sequence(points[:1])[2].shape == (6, 1) and disc.shared_sequence([]) is None
    # one flipped bit in one point's TEMP
    t2 = temp.copy()
    t2.view(np.uint64)[3] ^= np.uint64(1)
    assert t2[3] != temp[3] and abs(t2[3] - temp[3]) < 1e-13
    assert disc.shared_sequence(points[:2] + [_point(press.copy(), t2, scales[2])]) is None
    # ... and each of the other things the points must share
    for change in ("PRESS", "AMOUNT", "DTE", "DAM", "DCO"):
        p = _point(press.copy(), temp.copy(), scales[2])
        getattr(p[0], change).reshape(-1)[0] *= 1.0 + 2.0 ** -52
        assert disc.shared_sequence(points[:2] + [p]) is None, change
    p = _point(press.copy(), temp.copy(), scales[2])
    p[1].LAYINC = p[1].LAYINC[::-1].copy()
    assert disc.shared_sequence(points[:2] + [p]) is None
    p = _point(press.copy(), temp.copy(), scales[2])
    p[1].NLAYIN = np.array([5])
    assert disc.shared_sequence(points[:2] + [p]) is None
    assert disc.shared_sequence(points[:2] + [_point(press.copy(), temp.copy(), scales[2], tsurf=180.0)]) is None
    p = _point(press.copy(), temp.copy(), scales[2])
    assert disc.shared_sequence(points[:2] + [(p[0], p[1], p[2], p[3] * 2.0)]) is None           # xmap
    assert disc.shared_sequence([_point(press.copy(), temp.copy(), s, npath=2) for s in scales]) is None   # NPATH != 1


# ---- the adapter on the real reference, engine double ------------------------------------------------------------------
@pytest.fixture()
def disc_case(oracle, monkeypatch):
    """The cut C1 case as one geometry of an unresolved planet with three averaging points in a scratch directory, the reference
    imported, the adapter's engine replaced by the oracle double with the fused call restated un-collapsed."""
    import shutil
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.ref_import import import_reference
    from oracle import gen_golden_jacobian as gj
    from test_dropin_reference import OracleEngineDouble
    import archnemesis_dist_amd.forward_model as fmod

    class DiscEngineDouble(OracleEngineDouble):
        disc_calls = 0
        thg_calls = 0

        def cirsradg_ck_thermal(self, *a, **k):
            self.thg_calls += 1
            return super().cirsradg_ck_thermal(*a, **k)

        def cirsradg_ck_disc(self, ISPACE, lp, lt, am, taucont, dtaucon, NVMR, NPAR, igas_map, LAYINC, SCALE, EMTEMP, TSURF,
                             EMISSIVITY=None, mix=None, xfac=None, gradients_on_device=False, dtau_every_gas=None):
            N, P = np.shape(SCALE)
            spec, dspec, dts = OracleEngineDouble.cirsradg_ck_thermal(
                self, ISPACE, lp, lt, am, taucont, dtaucon, NVMR, NPAR, igas_map, np.full(P, N, dtype=np.int32),
                np.ascontiguousarray(np.tile(np.asarray(LAYINC)[:, None], (1, P))), SCALE,
                np.ascontiguousarray(np.tile(np.asarray(EMTEMP)[:, None], (1, P))), TSURF, EMISSIVITY=EMISSIVITY, xfac=xfac)
            MOD, dTSMOD, dMOD = dc.mod_from_points(spec, dspec, dts, np.asarray(mix), np.asarray(LAYINC), len(lp))
            self.disc_calls += 1
            self._dmod = dMOD
            xf = 1.0 if xfac is None else np.asarray(xfac)[:, None]
            return MOD, spec / xf, dTSMOD, (None if gradients_on_device else dMOD)

        def map2pro(self, dSPECIN, *a, to_host=True, **k):
            out = self.orc.map2pro(self._dmod if dSPECIN is None else dSPECIN, *a, **k)
            self._pro = out
            return out if to_host else None

        def map2xvec(self, dSPECIN, *a, **k):
            return self.orc.map2xvec(self._pro if dSPECIN is None else dSPECIN, *a, **k)

    ans = import_reference()
    work = tempfile.mkdtemp(prefix="ansfm_disc_")
    gj.setup_c1(ans, work)
    cwd = os.getcwd()
    os.chdir(work)
    double = DiscEngineDouble(oracle)
    monkeypatch.setattr(fmod, "get_engine", lambda device=0: double)
    fmod.set_strict(True)
    fmod.reset_summary()

    def make(cls=None, emiss_ang=EMISS_ANG, surface=False):
        fm = gj.cut_case(ans, cls=cls, nkeep=10, free=(20, 45, 70))
        if surface:                                       # the second capture of the generator: 180 K, a rising emissivity
            S = fm.Surface
            S.GASGIANT, S.NLOCATIONS, S.TSURF, S.NEM = False, 1, np.float64(180.0), 2
            S.VEM, S.EMISSIVITY = np.array([0.0, 40.0]), np.array([0.55, 0.95])
        M = fm.Measurement                                # as tools/golden/gen_golden_disc.py sets the case up
        nav = WGEOM.shape[1]
        M.NGEOM = 1
        M.NAV = np.array([nav], dtype="int32")
        z = np.zeros((1, nav))
        M.FLAT, M.FLON, M.AZI_ANG, M.TANHE = z.copy(), z.copy(), z.copy(), z.copy()
        M.SOL_ANG = np.full((1, nav), 60.0)
        M.EMISS_ANG = np.array(emiss_ang, dtype=float)
        M.WGEOM = WGEOM.copy()
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
    err = np.abs(dspec - ref).max(axis=(0, 1)) / np.where(scale > 0, scale, 1.0)
    print("columns by err:", np.array2string(err[scale > 0], precision=2))
    assert np.all(err[scale > 0] <= np.broadcast_to(tol, err.shape)[scale > 0])
    assert np.all(dspec[:, :, scale == 0] == 0.0)


@_mark
@pytest.mark.parametrize("case", ["", "S_"])
def test_override_reproduces_the_golden_nemesisdiscfmg(disc_case, golden_dir, case):
    """(SPECONV, dSPECONV) of the override against the reference's own nemesisdiscfmg() in the fixture, without a surface and
    (S_) with the surface at 180 K through the TSURF > 0 branch and convg: SPECONV rtol 2e-7 (float32 table grids, as in
    test_jacobian_dropin.py); every column of dSPECONV within 1e-8 of its largest element, the bound test_limb_host.py asks of
    the same comparison, plus the allowance derived in dc.cancellation_terms for the rounding of T_{j-1} - T_j and of T_end.
    That allowance comes to 1.43e-4 for the topmost temperature level of this case, beyond the Jacobian contract of 1e-4 the
    issue wanted it to stay within; a column's tolerance is therefore min(1e-8 + allowance, 1e-4).  Without a surface the same
    through jacobian_nemesis(nemesisdisc=True, analytical_gradient=True); exactly one fused call each and no un-collapsed one,
    the route counted, nothing delegated under set_strict(True)."""
    ans, fmod, double, make = disc_case
    z = np.load(os.path.join(golden_dir, "disc_c1.npz"))
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    spec, dspec = _quiet(make(FMGPU, surface=bool(case)).nemesisdiscfmg)
    assert double.disc_calls == 1 and double.thg_calls == 0
    ref_spec, ref_dspec = z[case + "SPECONV"], z[case + "dSPECONV"]
    assert spec.shape == ref_spec.shape and dspec.shape == ref_dspec.shape
    np.testing.assert_allclose(spec, ref_spec, rtol=2e-7)
    allowance = 4.0 * 2.0 ** -53 * dc.golden_cancellation_by_column(z, double.orc, case)[0]
    _columns_agree(dspec, ref_dspec, np.minimum(1e-8 + allowance, 1e-4))              # never beyond the Jacobian contract
    routes = fmod.summary()["routes"]
    assert routes.get("nemesisdiscfmg: averaging points mixed on the device") == 1 and fmod.summary()["delegated"] == {}
    if case:
        assert np.abs(spec - z["SPECONV"]).max() > 0                                  # the surface is in the spectrum
        return
    fm = make(FMGPU)
    YN, KK = _quiet(fm.jacobian_nemesis, NCores=1, nemesisdisc=True, analytical_gradient=True)
    assert double.disc_calls == 2 and double.thg_calls == 0 and fmod.summary()["delegated"] == {}
    nc = int(fm.Measurement.NCONV[0])
    assert np.array_equal(YN, spec[:nc, 0])
    analytic = np.asarray(fm.Variables.NUM) == 0
    assert analytic.any() and np.array_equal(KK[:, analytic], dspec[:nc, 0, :][:, analytic])


@_mark
def test_override_puts_the_mixed_surface_gradient_into_its_column(disc_case, monkeypatch):
    """With a stand-in JSURF >= 0 the column of the state vector that holds the surface temperature is overwritten with dTSMOD
    (:2062-2063 carried through the weighted sum); the other columns are what they are without it."""
    ans, fmod, double, make = disc_case
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    seen = {}
    orig_convg = type(make(FMGPU).Measurement).convg

    def convg(self, WAVE, SPEC, dSPEC, **k):
        seen["dSPEC"] = np.array(dSPEC)
        return orig_convg(self, WAVE, SPEC, dSPEC, **k)

    orig_disc = type(double).cirsradg_ck_disc

    def disc_call(self, *a, **k):
        out = orig_disc(self, *a, **k)
        seen["dTSMOD"] = np.array(out[2])
        return out

    monkeypatch.setattr(type(make(FMGPU).Measurement), "convg", convg)
    monkeypatch.setattr(type(double), "cirsradg_ck_disc", disc_call)
    _quiet(make(FMGPU).nemesisdiscfmg)
    plain = seen["dSPEC"]
    fm = make(FMGPU)
    fm.Variables.JSURF = 7
    _quiet(fm.nemesisdiscfmg)
    assert np.abs(seen["dTSMOD"]).min() > 0
    assert np.array_equal(seen["dSPEC"][:, 7], seen["dTSMOD"][:, 0]) and not np.array_equal(plain[:, 7], seen["dSPEC"][:, 7])
    rest = np.arange(plain.shape[1]) != 7
    assert np.array_equal(seen["dSPEC"][:, rest], plain[:, rest])


@_mark
def test_override_hands_every_case_it_does_not_take_to_process_IAV_or_the_reference_method(disc_case, monkeypatch):
    """A Telluric object and an engine without the call: the reference's method.  A point with EMISS_ANG < 0, points whose layers
    differ, a case _ansfm_supported(True) declines, a path calculation that is not thermal emission and runtime line-by-line: the
    points one by one through process_IAV in this process, weighted as :1789-1794 -- never an error, never a fused call."""
    ans, fmod, double, make = disc_case
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    seen, points = [], []
    monkeypatch.setattr(ans.ForwardModel_0, "nemesisdiscfmg", lambda self: seen.append(1) or "reference")
    fm = make(FMGPU)
    fm.Telluric = object()
    assert fm.nemesisdiscfmg() == "reference" and len(seen) == 1

    def process_IAV(self, IAV, IGEOM, return_grad=False):
        points.append((IGEOM, IAV, return_grad))
        W = self.SpectroscopyX.NWAVE
        return np.full(W, 10.0 ** IAV), np.full((W, self.Variables.NX), 10.0 ** IAV)

    monkeypatch.setattr(ans.ForwardModel_0, "process_IAV", process_IAV)
    captured = {}
    MeasCls = type(make(FMGPU).Measurement)
    orig_convg = MeasCls.convg

    def convg(self, WAVE, SPEC, dSPEC, **k):
        captured["SPEC"], captured["dSPEC"], captured["kw"] = np.array(SPEC), np.array(dSPEC), k
        return orig_convg(self, WAVE, SPEC, dSPEC, **k)

    monkeypatch.setattr(MeasCls, "convg", convg)
    orig_paths = ans.ForwardModel_0.calc_pathg

    def after_paths(change):
        def calc_pathg(self, *a, **k):
            out = orig_paths(self, *a, **k)
            change(self)
            return out
        return calc_pathg

    def runtime_lbl(self):
        self.SpectroscopyX.ILBL = fmod.ILBL_LBL_RUNTIME          # no LINE_DATA: _ansfm_line_source declines

    def not_thermal(self):
        self.PathX.IMOD = np.zeros_like(np.asarray(self.PathX.IMOD))      # pure transmission

    count = [0]

    def other_layers(self):
        count[0] += 1
        if count[0] == 2:                                        # the second point's layers differ in one bit
            T = np.array(self.LayerX.TEMP)
            T.view(np.uint64)[5] ^= np.uint64(1)
            self.LayerX.TEMP = T

    def expect_fallback(n_before, what):
        assert points[n_before:] == [(0, 0, True), (0, 1, True), (0, 2, True)], what
        assert np.allclose(captured["SPEC"], 0.2 + 5.0 + 30.0) and np.allclose(captured["dSPEC"], 35.2), what
        assert captured["kw"]["IGEOM"] == 0 and "FWHMEXIST" in captured["kw"], what

    _quiet(make(FMGPU, emiss_ang=[[0.0, -1.0, 65.0]]).nemesisdiscfmg)
    expect_fallback(0, "EMISS_ANG < 0")
    for change in (other_layers, not_thermal, runtime_lbl):
        n = len(points)
        monkeypatch.setattr(ans.ForwardModel_0, "calc_pathg", after_paths(change))
        fm = make(FMGPU)
        if change is runtime_lbl:
            monkeypatch.setattr(type(fm.Measurement), "lblconvg", lambda self, W, S, d, **k: convg(self, W, S, d, FWHMEXIST='', **k),
                                raising=False)
        _quiet(fm.nemesisdiscfmg)
        expect_fallback(n, change.__name__)
    monkeypatch.setattr(ans.ForwardModel_0, "calc_pathg", orig_paths)
    with monkeypatch.context() as m:
        m.setattr(fmod.CIRSradGPU, "_ansfm_supported", lambda self, return_grad: False)
        n = len(points)
        _quiet(make(FMGPU).nemesisdiscfmg)
        expect_fallback(n, "_ansfm_supported")
    assert double.disc_calls == 0 and len(seen) == 1 and fmod.summary()["delegated"] == {}
    monkeypatch.delattr(type(double), "cirsradg_ck_disc")
    assert make(FMGPU).nemesisdiscfmg() == "reference" and len(seen) == 2


@_mark
def test_override_falls_back_when_the_engine_answers_unsupported(disc_case, monkeypatch):
    """An engine that refuses the fused call (more than 160 layers, no room for dMOD or the scratch: NotImplementedError) sends
    the geometry's points through process_IAV, whose CIRSrad(return_grad=True) runs on the same engine; the fallback is noted
    once in summary(), not counted as the fused route, and gives the numbers of the fused route."""
    ans, fmod, double, make = disc_case
    FMGPU = fmod.make_gpu_forward_model(ans.ForwardModel_0)
    fused = _quiet(make(FMGPU).nemesisdiscfmg)
    fmod.reset_summary()
    refused = []

    def unsupported(self, *a, **k):
        refused.append(1)
        raise NotImplementedError("cirsradg_ck_disc: ANSFM_ERR_UNSUPPORTED")

    monkeypatch.setattr(type(double), "cirsradg_ck_disc", unsupported)
    assert double.thg_calls == 0
    with pytest.warns(RuntimeWarning, match="fused disc call"):
        spec, dspec = make(FMGPU).nemesisdiscfmg()
    assert refused == [1] and double.thg_calls == 3                      # CIRSrad(return_grad=True) of every point
    summ = fmod.summary()
    assert any("fused disc call" in k for k in summ["notes"]) and not any("nemesisdiscfmg" in k for k in summ["routes"])
    assert summ["delegated"] == {}
    # the same opacities and the same gradients either way; only the order of the linear sums over points, layers and levels
    # differs: 1e-12 of a column's largest element
    np.testing.assert_allclose(spec, fused[0], rtol=1e-12)
    _columns_agree(dspec, fused[1], 1e-12)
