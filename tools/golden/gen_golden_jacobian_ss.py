"""Jacobian-harness golden for the single-scattering configuration: the REFERENCE's own `jacobian_nemesis` on its scattering test
inputs (tests/files/Jupiter_CIRS_angled_thermal_emission_scattering) with ISCAT = 3 (SINGLE_SCATTERING_PLANE_PARALLEL: NUM[:] = 1,
every free element costs one forward model, ForwardModel_0.py:2251-2252), synthetic k-tables (seed 4, as
oracle/gen_golden_jacobian_ms.py), cut to NKEEP convolution points and eight free elements: six temperature levels (model 0) and
two parameters of the aerosol profile (model 47).

As shipped the case is useless for this branch: Jupiter at 9.5 AU scatters at most 2e-5 of the radiance.  The points are
therefore taken from the 1200 cm-1 end (VCONV[FIRST : FIRST + NKEEP]) and the star is moved closer (Stellar.DIST / 300); the
share of the solar terms in the unperturbed spectrum, 1 - SPEC(SOLFLUX = 0) / SPEC per (wavenumber, g), is computed with the
reference's own calc_singlescatt_plane_spectrum, kept as SOLAR_SHARE and asserted to have a median of at least 0.1.

Kept: xnx, ixrun, inum, XN, FIX, YN, KK and for every forward model what CIRSrad's single-scattering branch read (layer
properties, TAUCIA + TAUDUST + TAURAY, TAURAY + TAUSCAT, the layer-mean phase function per path, SCALE, EMTEMP) and returned;
once, the static arrays.  Build container only.

    python tools/golden/gen_golden_jacobian_ss.py        # -> tests/golden/jacobian_ss.npz
"""
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle.ref_import import import_reference, REFERENCE_ROOT  # noqa: E402
from oracle import gen_golden_jacobian as gj  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CASE = "Jupiter_CIRS_angled_thermal_emission_scattering"
NKEEP = 24
FIRST = 500
FREE = (6, 12, 20, 30, 40, 48, 81, 82)
ISCAT_SINGLE = 3
DIST_DIVISOR = 300.0


def cut_case(ans, cls=None):
    """gj.cut_case, then the NKEEP points from FIRST on, the star closer, ISCAT = 3"""
    FM = gj.cut_case(ans, cls=cls, nkeep=FIRST + NKEEP, free=FREE)
    M = FM.Measurement
    M.NCONV = np.array([NKEEP], dtype="int32")
    M.VCONV = M.VCONV[FIRST:]; M.MEAS = M.MEAS[FIRST:]; M.ERRMEAS = M.ERRMEAS[FIRST:]
    M.NY = NKEEP
    FM.Stellar.DIST = FM.Stellar.DIST / DIST_DIVISOR
    FM.Scatter.ISCAT = ISCAT_SINGLE
    return FM


def main():
    ans = import_reference()
    fm_mod = sys.modules["archnemesis.ForwardModel_0"]
    work = tempfile.mkdtemp(prefix="ansfm_jacss_")
    gj.setup_c1(ans, work, seed=4, case=CASE)
    calls = []
    o_cirs, o_ss, o_cia = fm_mod.ForwardModel_0.CIRSrad, fm_mod.calc_singlescatt_plane_spectrum, fm_mod.ForwardModel_0.calculate_vertical_cia_opacity
    pend = {}

    def w_ss(*a):
        res = o_ss(*a)
        pend.setdefault("ss", []).append((tuple(np.array(x) for x in a), np.array(res)))
        return res

    def w_cia(self, return_grad=False):
        r = o_cia(self, return_grad)
        pend["cia"] = r[0]
        return r

    def w_cirs(self, return_grad=False):
        pend["ss"] = []
        res = o_cirs(self, return_grad)
        S, L, P, A, Sc = self.SpectroscopyX, self.LayerX, self.PathX, self.AtmosphereX, self.ScatterX
        igas = np.array([A.locate_gas(S.ID[i], S.ISO[i]) for i in range(S.NGAS)])
        NPATH, ND = int(P.NPATH), int(Sc.NDUST)
        assert len(pend["ss"]) == NPATH
        # the layer-mean phase function of every path by LAYER, as :4259-4321 forms it, checked against what the layer loop read
        rad = np.pi / 180.
        calpha = np.sin(P.SOL_ANG * rad) * np.sin(P.EMISS_ANG * rad) * np.cos(P.AZI_ANG * rad - np.pi) - np.cos(P.EMISS_ANG * rad) * np.cos(P.SOL_ANG * rad)
        alpha = np.arccos(calpha) / np.pi * 180.
        pf_d, pf_r = Sc.calc_phase(alpha, S.WAVE), Sc.calc_phase_ray(alpha)
        PHASE = np.zeros((NPATH, S.NWAVE, L.NLAY))
        for ip in range(NPATH):
            ph = np.sum(pf_d[:, ip, :][:, None, :] * L.TAUCLSCAT, axis=2) + pf_r[ip] * L.TAURAY
            pos = ph > 0
            ph[pos] = ph[pos] / (L.TAURAY[pos] + L.TAUSCAT[pos])
            PHASE[ip] = ph
            n = int(P.NLAYIN[ip])
            np.testing.assert_allclose(ph[:, P.LAYINC[:n, ip]], pend["ss"][ip][0][5], rtol=1e-13, atol=0)
        calls.append(dict(XN=np.array(self.Variables.XN), PRESS=np.array(L.PRESS), TEMP=np.array(L.TEMP), AMOUNT=np.array(L.AMOUNT[:, igas]),
                          TAUCONT=np.array(pend["cia"]) + L.TAUDUST + L.TAURAY, TAUSCA=L.TAURAY + L.TAUSCAT, PHASE=PHASE,
                          SCALE=np.array(P.SCALE), EMTEMP=np.array(P.EMTEMP), SPECOUT=np.array(res)))
        if len(calls) == 1:
            a = pend["ss"][0][0]
            # share of the solar terms (singly scattered and surface-reflected sunlight) in the unperturbed state, per (wavenumber, g)
            dark = o_ss(*a[:9], np.zeros_like(a[9]), *a[10:])
            share = 1.0 - dark / pend["ss"][0][1]
            calls[0]["static"] = dict(
                WAVE=np.array(S.WAVE), K=np.array(S.K), TPRESS=np.array(S.PRESS), TTEMP=np.array(S.TEMP), DELG=np.array(S.DELG),
                NLAYIN=np.array(P.NLAYIN), LAYINC=np.array(P.LAYINC), IMOD=np.array(P.IMOD).astype(int), SOL_ANG=np.array(P.SOL_ANG),
                EMISS_ANG=np.array(P.EMISS_ANG), AZI_ANG=np.array(P.AZI_ANG), TSURF=float(self.SurfaceX.TSURF),
                ISPACE=int(self.MeasurementX.ISPACE), IFORM=int(self.MeasurementX.IFORM), SOLFLUX=np.array(a[9]),
                EMISSIVITY=np.array(a[7]), BRDF=np.stack([c[0][8] for c in pend["ss"]], axis=1), SOLAR_SHARE=share)
        return res

    cwd = os.getcwd()
    os.chdir(work)
    try:
        fm_mod.ForwardModel_0.CIRSrad = w_cirs
        fm_mod.calc_singlescatt_plane_spectrum = w_ss
        fm_mod.ForwardModel_0.calculate_vertical_cia_opacity = w_cia
        FM = cut_case(ans)
        XN0 = np.array(FM.Variables.XN)
        t = time.time()
        YN, KK = FM.jacobian_nemesis(NCores=1, analytical_gradient=True)       # ISCAT = 3 forces the numerical route anyway
        print("reference jacobian_nemesis(NCores=1): %.1f s, %d forward models" % (time.time() - t, len(calls)))
        V, M = FM.Variables, FM.Measurement
        assert np.all(V.NUM == 1)
        inum = np.where((V.NUM == 1) & (V.FIX == 0))[0]
        ixrun = np.concatenate([[0], inum + 1]).astype("int32")
        assert len(calls) == len(ixrun)
        xnx = np.zeros((V.NX, V.NX + 1)); xnx[:, 0] = XN0
        xnx[:, 1:] = np.repeat(XN0[:, None], V.NX, axis=1) + np.diag(0.05 * XN0)
        blk = xnx[:, 1:]; blk[blk == 0] = 0.05
        for c, ix in zip(calls, ixrun):
            assert np.array_equal(c["XN"], xnx[:, ix])
        st = calls[0].pop("static")
        assert int(st["IMOD"][0]) & 1024 and not int(st["IMOD"][0]) & 64
        share = st["SOLAR_SHARE"]
        print("solar share of the unperturbed state: median %.3f, max %.3f" % (np.median(share), share.max()))
        assert np.median(share) >= 0.1
        stack = lambda k: np.stack([c[k] for c in calls])
        VCONV = np.array(M.VCONV[:NKEEP, 0])
        YNtot = np.stack([np.interp(VCONV, st["WAVE"], c["SPECOUT"][:, 0]) for c in calls], axis=1)
        assert np.allclose(YNtot[:, 0], YN, rtol=1e-13, atol=0)
        # NCores = 1 leaves Variables.XN at the last perturbed state (see oracle/gen_golden_jacobian.py): the last free column
        # of KK comes out divided by 1.05.  Kept as the two-worker run has it.
        KK = np.array(KK)
        KK[:, inum[-1]] *= 1.05
        assert np.all(np.abs(KK[:, inum]).max(axis=0) > 0)
        for i, ix in enumerate(inum):              # every column is the quotient of this run's own spectra (:2355-2359)
            np.testing.assert_allclose(KK[:, ix], (YNtot[:, i + 1] - YNtot[:, 0]) / (xnx[ix, ix + 1] - xnx[ix, 0]), rtol=1e-9, atol=0)
        out = dict(xnx=xnx, ixrun=ixrun, inum=inum, XN=XN0, FIX=np.array(V.FIX), YN=YN, KK=KK, YNtot=YNtot, VCONV=VCONV,
                   LAY_PRESS=stack("PRESS"), LAY_TEMP=stack("TEMP"), LAY_AMOUNT=stack("AMOUNT"), TAUCONT=stack("TAUCONT"),
                   TAUSCA=stack("TAUSCA"), PHASE=stack("PHASE"), SCALE=stack("SCALE"), EMTEMP=stack("EMTEMP"), SPECOUT=stack("SPECOUT"),
                   **st)
    finally:
        os.chdir(cwd)
        fm_mod.ForwardModel_0.CIRSrad = o_cirs
        fm_mod.calc_singlescatt_plane_spectrum = o_ss
        fm_mod.ForwardModel_0.calculate_vertical_cia_opacity = o_cia
        shutil.rmtree(work, ignore_errors=True)
    fn = os.path.join(OUT, "jacobian_ss.npz")
    np.savez_compressed(fn, **out)
    print("wrote", fn, "%.2f MB" % (os.path.getsize(fn) / 1e6), "KK", KK.shape, "free columns", [int(i) for i in inum])


if __name__ == "__main__":
    main()
