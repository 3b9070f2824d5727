"""Primary-transit golden: the REFERENCE's own `nemesisPTfm(gradients=True)` (ForwardModel_0.py:1838-1995) on the cut C1 case
of oracle/gen_golden_jacobian.py (10 convolution points, 9 calculation wavenumbers, 71 layers -> 70 limb paths, one model-0
temperature profile of 81 levels) with IFORM = TransitDepth.  Kept: what `AnsfmEngine.cirsradg_ck_transit` needs (table slice and
grids, layers, continuum and its gradients, paths), the reference's TAUTOT / dTAUTOT of the layers, what the maps need (DTE / DAM
/ DCO, xmap, incpar), the reference's SPECOUT, its SPECMOD / dSPECMOD as handed to convg, its SPECONV / dSPECONV, and per column
the error of the NumPy restatement (tests/transit_cases.py) against dSPECMOD.  Build container only.

    python tools/golden/gen_golden_transit.py        # -> tests/golden/transit_c1.npz
"""
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.ref_import import import_reference  # noqa: E402
from oracle import gen_golden_jacobian as gj  # noqa: E402
from oracle import oracle as orc  # noqa: E402
import transit_cases as tc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "transit_c1.npz")
FREE = (20, 45, 70)


def main():
    ans = import_reference()
    FM = sys.modules["archnemesis.ForwardModel_0"].ForwardModel_0
    MEAS = sys.modules["archnemesis.Measurement_0"].Measurement_0
    work = tempfile.mkdtemp(prefix="ansfm_transit_")
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
                   BASEH=np.array(L.BASEH), RADIUS=float(A.RADIUS), RSTAR_KM=float(self.StellarX.RADIUS),
                   DTE=np.array(L.DTE), DAM=np.array(L.DAM), DCO=np.array(L.DCO), NVMR=int(A.NVMR), NDUST=int(A.NDUST), NPRO=int(A.NP),
                   SPECOUT=np.array(res[0]))
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

    cwd = os.getcwd()
    os.chdir(work)
    FM.CIRSrad, FM.calculate_gaseous_line_opacity, MEAS.convg, FM.subprofretg = cirsrad, gas, convg, subprofretg
    try:
        fm = gj.cut_case(ans, nkeep=10, free=FREE)
        fm.Measurement.IFORM = 2
        t = time.time()
        SPECONV, dSPECONV = fm.nemesisPTfm(gradients=True)
        print("reference nemesisPTfm(gradients=True): %.1f s (with the two extra opacity passes of the capture)" % (time.time() - t))
        VCONV = np.array(fm.Measurement.VCONV[:10, 0])
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
    tan = tc.tangent_heights_km(z["BASEH"], z["NLAYIN"], z["LAYINC"])
    c = tc.path_weights(tan, z["RADIUS"])
    Sm = tc.path_matrix(L, z["NLAYIN"], z["LAYINC"], z["SCALE"])
    delg = np.asarray(z["DELG"], dtype=np.float64)
    AREA, TRANS, dAREA = tc.collapsed(z["TAUTOT"], delg, Sm, c, z["dTAUTOT"])
    spec, fac = tc.depth(AREA, z["RADIUS"], tan[0], z["RSTAR_KM"])
    W = spec.size
    pro = orc.map2pro(dAREA[..., None], W, NVMR, NDUST, NPRO, 1, np.array([L]), np.arange(L)[:, None], z["DTE"], z["DAM"], z["DCO"],
                      INCPAR=list(incpar))
    dspec = orc.map2xvec(pro, W, NVMR, NDUST, NPRO, 1, NX, xmap)[:, 0, :] * fac
    ref = z["dSPECMOD"][:, 0, :]
    scale = np.abs(ref).max(axis=0)
    err = np.abs(dspec - ref).max(axis=0) / np.where(scale > 0, scale, 1.0)
    print("restatement: SPECMOD max |diff| %.3e, TRANS vs SPECOUT %.3e, dSPECMOD worst column %.3e of its largest element, %d non-zero columns"
          % (np.abs(spec - z["SPECMOD"][:, 0]).max(), np.abs(TRANS - z["SPECOUT"]).max(), err.max(), int(np.count_nonzero(scale))))
    np.savez_compressed(OUT, **z, incpar=incpar, VCONV=VCONV, SPECONV=np.array(SPECONV), dSPECONV=np.array(dSPECONV),
                        restatement_err=err, FREE=np.array(FREE))
    print("wrote", OUT, "%.2f MB" % (os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
