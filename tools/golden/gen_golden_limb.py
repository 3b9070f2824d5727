"""Limb-emission golden: the REFERENCE's own `nemesisLfmg()` (ForwardModel_0.py:1372-1521) on the cut C1 case of
oracle/gen_golden_jacobian.py (10 convolution points, 9 calculation wavenumbers, 71 layers, one model-0 temperature profile of
81 levels) set up as a limb observation of three geometries at tangent heights 40 / 80 / 130 km, for which calc_pathg_L makes the
six limb paths that bracket them.  Captured the way tools/golden/gen_golden_occultation.py captures its case, plus EMTEMP of the
paths and ISPACE: what `AnsfmEngine.cirsradg_ck_limb` needs (table slice and grids, layers, continuum and its gradients, paths,
TANHE, the unit factor), the reference's TAUTOT / dTAUTOT of the layers, what the maps need (DTE / DAM / DCO, xmap, incpar), the
reference's SPECOUT, its SPECMOD / dSPECMOD as handed to convg, its SPECONV / dSPECONV, and per column the error of the NumPy
restatement (tests/limb_cases.py) against dSPECMOD.  Only data goes into the file.  Build container only.

    python tools/golden/gen_golden_limb.py        # -> tests/golden/limb_c1.npz
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
import limb_cases as lc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "limb_c1.npz")
FREE = (20, 45, 70)
TANHE = [[40.0], [80.0], [130.0]]


def main():
    ans = import_reference()
    FM = sys.modules["archnemesis.ForwardModel_0"].ForwardModel_0
    MEAS = sys.modules["archnemesis.Measurement_0"].Measurement_0
    work = tempfile.mkdtemp(prefix="ansfm_limb_")
    gj.setup_c1(ans, work)
    rec = {}
    orig_cirs, orig_gas, orig_convg, orig_sub = FM.CIRSrad, FM.calculate_gaseous_line_opacity, MEAS.convg, FM.subprofretg
    zero_gas = [False]

    def gas(self, return_grad=False):
        tau, dtau = orig_gas(self, return_grad)
        return tau, (np.zeros_like(dtau) if zero_gas[0] and dtau is not None else dtau)

    def cirsrad(self, return_grad=False):
        res = orig_cirs(self, return_grad)
        S, L, P, A = self.SpectroscopyX, self.LayerX, self.PathX, self.AtmosphereX
        igas = np.array([A.locate_gas(S.ID[i], S.ISO[i]) for i in range(S.NGAS)])
        rec.update(WAVE=np.array(S.WAVE), K=np.array(S.K), TPRESS=np.array(S.PRESS), TTEMP=np.array(S.TEMP), DELG=np.array(S.DELG),
                   LAY_PRESS=np.array(L.PRESS), LAY_TEMP=np.array(L.TEMP), LAY_AMOUNT=np.array(L.AMOUNT[:, igas]),
                   TAUCONT=L.TAUCIA + L.TAUDUST + L.TAURAY, TAUTOT=np.array(L.TAUTOT), igas_map=igas.astype(np.int32),
                   NLAYIN=np.array(P.NLAYIN, dtype=np.int32), LAYINC=np.array(P.LAYINC, dtype=np.int32), SCALE=np.array(P.SCALE),
                   EMTEMP=np.array(P.EMTEMP), ISPACE=int(self.MeasurementX.ISPACE), IMOD=np.array(P.IMOD).astype(np.int32),
                   BASEH=np.array(L.BASEH), DTE=np.array(L.DTE), DAM=np.array(L.DAM), DCO=np.array(L.DCO), NVMR=int(A.NVMR),
                   NDUST=int(A.NDUST), NPRO=int(A.NP), SPECOUT=np.array(res[0]))
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
        rec["xmap"] = np.array(xmap)
        return xmap

    def convg(self, WAVE, SPECMOD, dSPECMOD, IGEOM="All"):
        rec.update(SPECMOD=np.array(SPECMOD), dSPECMOD=np.array(dSPECMOD))
        return orig_convg(self, WAVE, SPECMOD, dSPECMOD, IGEOM=IGEOM)

    def limb_case():
        """the cut C1 case as a limb observation: three geometries at 40 / 80 / 130 km"""
        fm = gj.cut_case(ans, nkeep=10, free=FREE)
        M = fm.Measurement
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
        M.TANHE = np.array(TANHE)
        M.WGEOM = np.ones((ng, 1))
        M.NY = n0 * ng
        return fm

    cwd = os.getcwd()
    os.chdir(work)
    FM.CIRSrad, FM.calculate_gaseous_line_opacity, MEAS.convg, FM.subprofretg = cirsrad, gas, convg, subprofretg
    try:
        fm = limb_case()
        t = time.time()
        SPECONV, dSPECONV = fm.nemesisLfmg()
        print("reference nemesisLfmg(): %.1f s (with the two extra opacity passes of the capture)" % (time.time() - t))
        VCONV = np.array(fm.Measurement.VCONV[:10, 0])
        xfac = np.ones(rec["WAVE"].size)
        if int(fm.MeasurementX.IFORM) == IFORM_FLUXRATIO:                        # :4158-4168
            import scipy.interpolate
            fm.StellarX.calc_solar_flux()
            xfac = xfac * np.pi * 4. * np.pi * ((fm.AtmosphereX.RADIUS) * 1.0e2) ** 2. / scipy.interpolate.interp1d(
                fm.StellarX.WAVE, fm.StellarX.SOLFLUX)(rec["WAVE"])
    finally:
        FM.CIRSrad, FM.calculate_gaseous_line_opacity, MEAS.convg, FM.subprofretg = orig_cirs, orig_gas, orig_convg, orig_sub
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)
    z = rec
    xmap = z["xmap"]
    NVMR, NDUST, NPRO = z["NVMR"], z["NDUST"], z["NPRO"]
    NPAR, NX, L = NVMR + 2 + NDUST, xmap.shape[0], z["LAY_PRESS"].size
    incpar = np.array([i for i in range(NPAR) if np.mean(xmap[:, i, :]) != 0.0], dtype=np.int32)
    # the restatement on the reference's own TAUTOT / dTAUTOT
    tan = lc.tangent_heights_km(z["BASEH"], z["NLAYIN"], z["LAYINC"])
    C = lc.tangent_mix(tan, TANHE)
    Q = C.shape[0]
    delg = np.asarray(z["DELG"], dtype=np.float64)
    assert all(lc.is_limb_path(z["LAY_PRESS"], z["NLAYIN"], z["LAYINC"], p) for p in range(len(z["NLAYIN"])))
    MOD, SPEC, dMOD = lc.collapsed(z["TAUTOT"], delg, z["NLAYIN"], z["LAYINC"], z["SCALE"], z["EMTEMP"], C, z["ISPACE"], z["WAVE"], NVMR,
                                   z["dTAUTOT"], xfac)
    W = MOD.shape[0]
    pro = orc.map2pro(dMOD, W, NVMR, NDUST, NPRO, Q, np.array([L] * Q), np.tile(np.arange(L)[:, None], (1, Q)), z["DTE"], z["DAM"],
                      z["DCO"], INCPAR=list(incpar))
    dspec = orc.map2xvec(pro, W, NVMR, NDUST, NPRO, Q, NX, xmap)                  # (W, Q, NX)
    ref = z["dSPECMOD"]
    scale = np.abs(ref).max(axis=(0, 1))                                          # (NX,): a column over wavenumbers and geometries
    err = np.abs(dspec - ref).max(axis=(0, 1)) / np.where(scale > 0, scale, 1.0)
    print("paths: NLAYIN %s, tangent heights %s km, IMOD %s, ISPACE %d" % (z["NLAYIN"], np.array2string(tan, precision=2), z["IMOD"],
                                                                           z["ISPACE"]))
    print("restatement: SPECMOD max rel diff %.3e, SPEC vs SPECOUT %.3e, dSPECMOD worst column %.3e of its largest element, %d of %d "
          "columns non-zero; SPECONV %.3e .. %.3e"
          % (np.abs(MOD / z["SPECMOD"] - 1).max(), np.abs(SPEC * xfac[:, None] / z["SPECOUT"] - 1).max(), err.max(),
             int(np.count_nonzero(scale)), scale.size, np.min(SPECONV), np.max(SPECONV)))
    # np.savez_compressed at the deflate level that keeps the file no larger than occultation_c1.npz (np.load reads it alike)
    arrays = dict(z, incpar=incpar, VCONV=VCONV, TANHE=np.array(TANHE), XFAC=xfac, SPECONV=np.array(SPECONV),
                  dSPECONV=np.array(dSPECONV), restatement_err=err, FREE=np.array(FREE))
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name, value in arrays.items():
            buf = io.BytesIO()
            np.save(buf, np.asanyarray(value))
            zf.writestr(name + ".npy", buf.getvalue())
    print("wrote", OUT, "%.2f MB" % (os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
