"""Disc-average golden: the REFERENCE's own `nemesisdiscfmg()` (ForwardModel_0.py:1719-1834) on the cut C1 case of
oracle/gen_golden_jacobian.py (10 convolution points, 9 calculation wavenumbers, 71 layers, one model-0 temperature profile of
81 levels) set up as one geometry of an unresolved planet with NAV = 3 averaging points at emission angles 0 / 40 / 65 degrees and
weights 0.2 / 0.5 / 0.3 (SOL_ANG 60, the other per-point arrays zero).  Captured the way tools/golden/gen_golden_limb.py captures
its case.  Per point: SCALE and CIRSrad's SPECOUT and dTSURF.  Once (the points agree in them bit for bit, asserted here): table
slice and grids, layers, continuum and its gradients, the layer sequence LAYINC / EMTEMP, the unit factor, the reference's TAUTOT /
dTAUTOT of the layers, what the maps need (DTE / DAM / DCO, xmap, incpar), SPEC / dSPEC as handed to convg, SPECONV / dSPECONV, and
per column the error of the NumPy restatement (tests/disc_cases.py) against dSPEC (restatement_err) and against sum WGEOM dTSURF
(restatement_err_dtsurf).  It also records that `nemesisfmg()` on the same model returns the same SPECONV / dSPECONV bit for bit
(fmg_equals_discfmg).

A second capture, keys prefixed "S_", is the same case with a surface: Surface.GASGIANT = False, TSURF = 180 K and an emissivity
that rises linearly from 0.55 at 0 cm-1 to 0.95 at 40 cm-1 (0.60 .. 0.78 on the calculation grid), so that the lower boundary
takes the branch of :6487-6491.  Only what differs from the first capture is stored for it (TSURF, EMISSIVITY on the calculation
grid, SPECOUT, dTSURF, SPEC / dSPEC as handed to convg, SPECONV / dSPECONV, the two restatement errors).  The table slice K holds
values read from float32 .kta files; it is stored as float32 where that changes no value (asserted), which keeps the file no
larger than limb_c1.npz.  Only data goes into the file.  Build container only.

    python tools/golden/gen_golden_disc.py        # -> tests/golden/disc_c1.npz
"""
import io
import os
import shutil
import sys
import tempfile
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.ref_import import import_reference  # noqa: E402
from oracle import gen_golden_jacobian as gj  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from archnemesis_dist_amd.forward_model import IFORM_FLUXRATIO  # noqa: E402
import disc_cases as dc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "disc_c1.npz")
FREE = (20, 45, 70)
EMISS_ANG = [[0.0, 40.0, 65.0]]
WGEOM = [[0.2, 0.5, 0.3]]
SHARED = ("LAY_PRESS", "LAY_TEMP", "LAY_AMOUNT", "TAUCONT", "TAUTOT", "LAYINC", "EMTEMP", "DTE", "DAM", "DCO", "xmap")


def disc_setup(fm):
    """the cut C1 case as one geometry of an unresolved planet with three averaging points"""
    M = fm.Measurement
    nav = len(WGEOM[0])
    M.NGEOM = 1
    M.NAV = np.array([nav], dtype="int32")
    z = np.zeros((1, nav))
    M.FLAT, M.FLON, M.AZI_ANG, M.TANHE = z.copy(), z.copy(), z.copy(), z.copy()
    M.SOL_ANG = np.full((1, nav), 60.0)
    M.EMISS_ANG = np.array(EMISS_ANG)
    M.WGEOM = np.array(WGEOM)
    return fm


def surface_setup(fm):
    S = fm.Surface
    S.GASGIANT = False
    S.NLOCATIONS = 1
    S.TSURF = np.float64(180.0)
    S.VEM = np.array([0.0, 40.0])                                             # the calculation grid is 5 .. 23 cm-1
    S.EMISSIVITY = np.array([0.55, 0.95])
    S.NEM = 2
    return fm


def main():
    ans = import_reference()
    FM = sys.modules["archnemesis.ForwardModel_0"].ForwardModel_0
    MEAS = sys.modules["archnemesis.Measurement_0"].Measurement_0
    work = tempfile.mkdtemp(prefix="ansfm_disc_")
    gj.setup_c1(ans, work)
    orig_cirs, orig_gas, orig_convg, orig_sub = FM.CIRSrad, FM.calculate_gaseous_line_opacity, MEAS.convg, FM.subprofretg
    zero_gas = [False]
    rec = {}

    def gas(self, return_grad=False):
        tau, dtau = orig_gas(self, return_grad)
        return tau, (np.zeros_like(dtau) if zero_gas[0] and dtau is not None else dtau)

    def cirsrad(self, return_grad=False):
        res = orig_cirs(self, return_grad)
        S, L, P, A = self.SpectroscopyX, self.LayerX, self.PathX, self.AtmosphereX
        assert int(P.NPATH) == 1
        n = int(np.asarray(P.NLAYIN).reshape(-1)[0])
        igas = np.array([A.locate_gas(S.ID[i], S.ISO[i]) for i in range(S.NGAS)])
        point = dict(LAY_PRESS=np.array(L.PRESS), LAY_TEMP=np.array(L.TEMP), LAY_AMOUNT=np.array(L.AMOUNT[:, igas]),
                     TAUCONT=L.TAUCIA + L.TAUDUST + L.TAURAY, TAUTOT=np.array(L.TAUTOT),
                     LAYINC=np.array(P.LAYINC, dtype=np.int32).reshape(-1)[:n], EMTEMP=np.array(P.EMTEMP).reshape(-1)[:n],
                     DTE=np.array(L.DTE), DAM=np.array(L.DAM), DCO=np.array(L.DCO), xmap=rec["xmap_now"],
                     SCALE=np.array(P.SCALE).reshape(-1)[:n], SPECOUT=np.array(res[0][:, 0]), dTSURF=np.array(res[2][:, 0]))
        rec.setdefault("points", []).append(point)
        if len(rec["points"]) > 1:
            return res
        rec.update(WAVE=np.array(S.WAVE), K=np.array(S.K), TPRESS=np.array(S.PRESS), TTEMP=np.array(S.TEMP), DELG=np.array(S.DELG),
                   igas_map=igas.astype(np.int32), ISPACE=int(self.MeasurementX.ISPACE), IMOD=np.array(P.IMOD).astype(np.int32),
                   NVMR=int(A.NVMR), NDUST=int(A.NDUST), NPRO=int(A.NP), TSURF=float(self.SurfaceX.TSURF),
                   JSURF=int(self.Variables.JSURF))
        if float(self.SurfaceX.TSURF) > 0:
            import scipy.interpolate
            rec["EMISSIVITY"] = scipy.interpolate.interp1d(self.SurfaceX.VEM, self.SurfaceX.EMISSIVITY)(S.WAVE)
        xfac = np.ones(rec["WAVE"].size)
        if int(self.MeasurementX.IFORM) == IFORM_FLUXRATIO:                        # :4158-4168
            import scipy.interpolate
            self.StellarX.calc_solar_flux()
            xfac = xfac * np.pi * 4. * np.pi * ((A.RADIUS) * 1.0e2) ** 2. / scipy.interpolate.interp1d(
                self.StellarX.WAVE, self.StellarX.SOLFLUX)(rec["WAVE"])
        rec["XFAC"] = xfac
        # the layers' own dTAUTOT and dTAUCON: calculate_layer_opacity once more on the identity path (x SCALE = 1 changes no bit),
        # the second time with the gas part zeroed (0 + dTAUCON)
        keep = P.NLAYIN, P.LAYINC, P.SCALE
        NLAY = int(L.NLAY)
        P.NLAYIN, P.LAYINC, P.SCALE = np.array([NLAY]), np.arange(NLAY)[:, None], np.ones((NLAY, 1))
        try:
            rec["dTAUTOT"] = np.array(self.calculate_layer_opacity(True)[2][..., 0])
            zero_gas[0] = True
            rec["dTAUCON"] = np.array(self.calculate_layer_opacity(True)[2][:, 0, :, :, 0])
        finally:
            zero_gas[0] = False
            P.NLAYIN, P.LAYINC, P.SCALE = keep
        return res

    def subprofretg(self, *a, **k):
        xmap = orig_sub(self, *a, **k)
        rec["xmap_now"] = np.array(xmap)
        return xmap

    def convg(self, WAVE, SPEC, dSPEC, **k):
        rec.update(SPEC=np.array(SPEC), dSPEC=np.array(dSPEC))
        return orig_convg(self, WAVE, SPEC, dSPEC, **k)

    def capture(surface):
        rec.clear()
        fm = disc_setup(gj.cut_case(ans, nkeep=10, free=FREE))
        if surface:
            surface_setup(fm)
        t = time.time()
        SPECONV, dSPECONV = fm.nemesisdiscfmg()
        print("reference nemesisdiscfmg(%s): %.1f s, %d CIRSrad calls (with the two extra opacity passes of the capture)"
              % ("surface" if surface else "", time.time() - t, len(rec["points"])))
        z = dict(rec)
        pts = z.pop("points"); z.pop("xmap_now")
        for k in SHARED:                                                         # bit for bit across the points
            assert all(np.asarray(p[k]).tobytes() == np.asarray(pts[0][k]).tobytes() for p in pts), k
            z[k] = pts[0][k]
        assert not all(np.array_equal(p["SCALE"], pts[0]["SCALE"]) for p in pts[1:])
        z["SCALE"] = np.stack([p["SCALE"] for p in pts], axis=1)                 # (N, NAV)
        z["SPECOUT"] = np.stack([p["SPECOUT"] for p in pts], axis=1)             # (W, NAV), times xfac
        z["dTSURF"] = np.stack([p["dTSURF"] for p in pts], axis=1)
        z.update(SPECONV=np.array(SPECONV), dSPECONV=np.array(dSPECONV), VCONV=np.array(fm.Measurement.VCONV[:10, 0]))
        rec.clear()
        fm2 = disc_setup(gj.cut_case(ans, nkeep=10, free=FREE))
        if surface:
            surface_setup(fm2)
        S2, dS2 = fm2.nemesisfmg()
        z["fmg_equals_discfmg"] = bool(np.array_equal(S2, SPECONV) and np.array_equal(dS2, dSPECONV))
        return z

    def restate(z):
        xmap = z["xmap"]
        NVMR, NDUST, NPRO = z["NVMR"], z["NDUST"], z["NPRO"]
        NPAR, NX, L = NVMR + 2 + NDUST, xmap.shape[0], z["LAY_PRESS"].size
        incpar = np.array([i for i in range(NPAR) if np.mean(xmap[:, i, :]) != 0.0], dtype=np.int32)
        C = np.array(WGEOM)
        delg = np.asarray(z["DELG"], dtype=np.float64)
        emis = z.get("EMISSIVITY") if z["TSURF"] > 0 else None
        MOD, SPEC, dTSMOD, dMOD = dc.collapsed(z["TAUTOT"], delg, z["LAY_PRESS"], z["LAYINC"], z["SCALE"], z["EMTEMP"], z["TSURF"], emis, C,
                                               z["ISPACE"], z["WAVE"], NVMR, z["dTAUTOT"], z["XFAC"])
        W = MOD.shape[0]
        pro = orc.map2pro(dMOD, W, NVMR, NDUST, NPRO, 1, np.array([L]), np.arange(L)[:, None], z["DTE"], z["DAM"], z["DCO"],
                          INCPAR=list(incpar))
        dspec = orc.map2xvec(pro, W, NVMR, NDUST, NPRO, 1, NX, xmap)[:, 0, :]      # (W, NX)
        ref = np.array(z["dSPEC"])
        if z["JSURF"] >= 0:
            dspec[:, z["JSURF"]] = dTSMOD[:, 0]
        scale = np.abs(ref).max(axis=0)
        err = np.abs(dspec - ref).max(axis=0) / np.where(scale > 0, scale, 1.0)
        ts_ref = z["dTSURF"] @ C[0]
        ts_err = np.abs(dTSMOD[:, 0] - ts_ref).max() / np.abs(ts_ref).max()
        print("sequence: N %d, ground %s, TSURF %g, JSURF %d, IMOD %s, ISPACE %d, SCALE[0] %s" % (
            z["LAYINC"].size, dc.is_ground(z["LAY_PRESS"], z["LAYINC"]), z["TSURF"], z["JSURF"], z["IMOD"], z["ISPACE"], z["SCALE"][0]))
        print("restatement: SPEC max rel diff %.3e, SPEC points vs SPECOUT %.3e, dSPEC worst column %.3e of its largest element, %d of %d "
              "columns non-zero; sum WGEOM dTSURF %.3e; SPECONV %.3e .. %.3e; nemesisfmg() equal bit for bit: %s"
              % (np.abs(MOD[:, 0] / z["SPEC"] - 1).max(), np.abs(SPEC * z["XFAC"][:, None] / z["SPECOUT"] - 1).max(), err.max(),
                 int(np.count_nonzero(scale)), scale.size, ts_err, np.min(z["SPECONV"]), np.max(z["SPECONV"]), z["fmg_equals_discfmg"]))
        z.update(incpar=incpar, restatement_err=err, restatement_err_dtsurf=ts_err)
        return z

    cwd = os.getcwd()
    os.chdir(work)
    FM.CIRSrad, FM.calculate_gaseous_line_opacity, MEAS.convg, FM.subprofretg = cirsrad, gas, convg, subprofretg
    try:
        plain = restate(capture(False))
        surf = restate(capture(True))
    finally:
        FM.CIRSrad, FM.calculate_gaseous_line_opacity, MEAS.convg, FM.subprofretg = orig_cirs, orig_gas, orig_convg, orig_sub
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)
    arrays = dict(plain, WGEOM=np.array(WGEOM[0]), EMISS_ANG=np.array(EMISS_ANG[0]), FREE=np.array(FREE))
    for k, v in surf.items():                                                   # what the surface changes, nothing else
        if k not in plain or np.asarray(v).tobytes() != np.asarray(plain[k]).tobytes():
            arrays["S_" + k] = v
    K32 = arrays["K"].astype(np.float32)
    if np.array_equal(K32.astype(np.float64), arrays["K"]):                     # float32 on file: nothing is lost
        arrays["K"] = K32
    print("second capture stores:", sorted(k for k in arrays if k.startswith("S_")))
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name, value in arrays.items():
            buf = io.BytesIO()
            np.save(buf, np.asanyarray(value))
            zf.writestr(name + ".npy", buf.getvalue())
    print("wrote", OUT, "%.2f MB" % (os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
