"""C4-LBL seam golden: the REFERENCE's CIRSrad with line-by-line tables (ILBL = 2) in its two scattering branches, on the
reference's own scattering test inputs (tests/files/Jupiter_CIRS_angled_thermal_emission_scattering: Rayleigh on, one
Henyey-Greenstein haze, sunlight on) with seeded synthetic .lta tables written by the reference's write_lbltable.

- multiple scattering (ISCAT = 1: calculate_multiple_scattering_spectrum -> scloud11wave -> scloud11wave_core): everything
  ansfm_cirsrad_ck_scatter takes, the table arrays (K, PRESS, TEMP, WAVE), TAUGAS, TAUTOT, the core's rad and SPECOUT (the
  core's taus and tauray are TAUTOT and TAURAY);
- single scattering, plane parallel (ISCAT = 3: calculate_single_scattering_plane_parallel_spectrum ->
  calc_singlescatt_plane_spectrum): the same layer inputs, what ansfm_cirsrad_ck_singlescatt takes (the per-path arguments
  of calc_singlescatt_plane_spectrum), TAUGAS, TAUTOT and SPECOUT.  Keys of this run carry the prefix ss_; what equals the
  multiple-scattering run's (layers, opacities, geometry) is stored once, without it.

The measurement is cut to NKEEP of its convolution points with a boxcar of FWHM wavenumbers (LBL tables need one): about a
hundred calculation wavenumbers, so that the un-jitted core finishes and the fixture stays small.  Needs the reference (build container only).

    python tools/golden/gen_golden_c4_lbl.py      # -> tests/golden/c4_lbl_scatter.npz
"""
import importlib
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_import import import_reference, REFERENCE_ROOT  # noqa: E402
from oracle.gen_golden_c1 import GASES  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
K0, NKEEP = 2, 2          # convolution points VCONV[K0:K0 + NKEEP]: the aerosol data start at 200 cm-1
FWHM = 2.5
VMIN, DELV, NWAVE_TAB = 190.0, 0.1, 280


def _write_tables(sp_mod, work):
    rng = np.random.default_rng(44)
    PRESS = np.logspace(-7, 1.2, 5); TEMP = np.linspace(70.0, 400.0, 4)
    names = []
    for name, gid, iso in GASES:
        base = 10.0 ** rng.uniform(-26, -21, size=(NWAVE_TAB, 1, 1))
        k = base * PRESS[None, :, None] ** 0.1 * (TEMP[None, None, :] / 200.0) ** 0.7
        fn = os.path.join(work, f"{name}_synth.lta")
        sp_mod.write_lbltable(fn, PRESS.size, TEMP.size, gid, iso, PRESS, TEMP, NWAVE_TAB, VMIN, DELV, k)
        names.append(fn)
    with open(os.path.join(work, "cirstest.lls"), "w") as f:
        f.write("\n".join(names) + "\n")


def _run(ans, fm_mod, ms_mod, work, iscat):
    with open(os.path.join(work, "cirstest.inp")) as f:
        lines = f.readlines()
    lines[0] = f"0 {iscat} 2\t\t\t! ISPACE, ISCAT, ILBL\n"
    with open(os.path.join(work, "cirstest.inp"), "w") as f:
        f.writelines(lines)
    cap = {"ss": []}
    o_cirs = fm_mod.ForwardModel_0.CIRSrad
    o_core = ms_mod.scloud11wave_core
    o_cia = fm_mod.ForwardModel_0.calculate_vertical_cia_opacity
    o_ss = fm_mod.calc_singlescatt_plane_spectrum

    def w_cirs(self, return_grad=False):
        res = o_cirs(self, return_grad)
        cap.setdefault("cirs", (self, res))
        return res

    def w_core(**kw):
        res = o_core(**kw)
        cap.setdefault("core", (dict(kw), res))
        return res

    def w_cia(self, return_grad=False):
        r = o_cia(self, return_grad)
        cap.setdefault("cia", r[0])
        return r

    def w_ss(*a):
        cap["ss"].append(a)
        return o_ss(*a)

    fm_mod.ForwardModel_0.CIRSrad = w_cirs
    ms_mod.scloud11wave_core = w_core
    fm_mod.ForwardModel_0.calculate_vertical_cia_opacity = w_cia
    fm_mod.calc_singlescatt_plane_spectrum = w_ss
    cwd = os.getcwd()
    os.chdir(work)
    try:
        Atm, Meas, Spec, Scat, Stel, Surf, CIA, Lay, Var, Ret = ans.Files.read_input_files("cirstest")
        Meas.NCONV = np.array([NKEEP], dtype="int32")
        keep = slice(K0, K0 + NKEEP)
        Meas.VCONV = Meas.VCONV[keep]; Meas.MEAS = Meas.MEAS[keep]; Meas.ERRMEAS = Meas.ERRMEAS[keep]
        Meas.NY = NKEEP
        Meas.FWHM = FWHM
        FM = ans.ForwardModel_0(runname="cirstest", Atmosphere=Atm, Surface=Surf, Measurement=Meas, Spectroscopy=Spec,
                                Stellar=Stel, Scatter=Scat, CIA=CIA, Layer=Lay, Variables=Var)
        t = time.time()
        SPECONV = FM.nemesisfm()
        print(f"nemesisfm (ISCAT = {iscat}, ILBL = 2)", time.time() - t, "s", SPECONV.shape)
        self, SPECOUT = cap["cirs"]
        S, L, P, A, Sc = self.SpectroscopyX, self.LayerX, self.PathX, self.AtmosphereX, self.ScatterX
        assert int(S.ILBL) == 2 and int(S.NG) == 1
        igas = np.array([A.locate_gas(S.ID[i], S.ISO[i]) for i in range(S.NGAS)])
        out = dict(
            SPECONV=SPECONV, WAVE=S.WAVE, K=S.K, TPRESS=S.PRESS, TTEMP=S.TEMP, ILBL=int(S.ILBL),
            LAY_PRESS=L.PRESS, LAY_TEMP=L.TEMP, LAY_AMOUNT=L.AMOUNT, IGAS=igas,
            TAUCIA=cap["cia"], TAURAY=L.TAURAY, TAUDUST=L.TAUDUST, TAUSCAT=L.TAUSCAT,
            TAUGAS=L.TAUGAS, TAUTOT=L.TAUTOT, IMOD=np.array(P.IMOD).astype(int),
            SOL_ANG=P.SOL_ANG, EMISS_ANG=P.EMISS_ANG, AZI_ANG=P.AZI_ANG,
            NLAYIN=np.asarray(P.NLAYIN), LAYINC=np.asarray(P.LAYINC), SCALE=np.asarray(P.SCALE), EMTEMP=np.asarray(P.EMTEMP),
            ISPACE=int(self.MeasurementX.ISPACE), IFORM=int(self.MeasurementX.IFORM),
            NMU=int(Sc.NMU), NF=int(Sc.NF), NPHI=int(Sc.NPHI), IRAY=int(Sc.IRAY), IMIE=int(Sc.IMIE), NDUST=int(Sc.NDUST),
            MU=Sc.MU, WTMU=Sc.WTMU, LOWBC=int(self.SurfaceX.LOWBC), GASGIANT=bool(self.SurfaceX.GASGIANT),
            TSURF=float(self.SurfaceX.TSURF), SPECOUT=SPECOUT)
        if "core" in cap:
            kw, rad = cap["core"]
            # the core's taus / tauray are LayerX.TAUTOT / TAURAY (scloud11wave :5099-5119): kept once, under those names
            assert np.array_equal(kw["taus"], L.TAUTOT) and np.array_equal(kw["tauray"], L.TAURAY)
            out.update(core_phasarr=np.ascontiguousarray(kw["phasarr"]), core_radg=kw["radg"], core_solar=kw["solar"],
                       core_brdf=kw["brdf_matrix"], core_bnu=kw["bnu"], core_omegas=kw["omegas_s"],
                       core_lfrac=np.ascontiguousarray(kw["lfrac"]), core_rad=rad)
        if cap["ss"]:
            # calc_singlescatt_plane_spectrum(ISPACE, WAVE, TAUTOT_PATH, TEMP, OMEGA, PHASE, TSURF, EMISSIVITY, BRDF, SOLFLUX,
            # SOL_ANG, EMISS_ANG) per path; PHASE (NWAVE, NLAYIN) is the layer-mean phase function on the path's layers
            npath = len(cap["ss"])
            W, NL = S.WAVE.size, L.NLAY
            phase = np.zeros((npath, W, NL))
            for ip, a in enumerate(cap["ss"]):
                nl = int(P.NLAYIN[ip])
                phase[ip][:, np.asarray(P.LAYINC)[0:nl, ip]] = a[5]
            out.update(ss_PHASE=phase, ss_EMISSIVITY=np.asarray(cap["ss"][0][7], dtype=np.float64),
                       ss_BRDF=np.stack([np.asarray(a[8], dtype=np.float64) for a in cap["ss"]], axis=1),
                       ss_SOLFLUX=np.asarray(cap["ss"][0][9], dtype=np.float64),
                       ss_TSURF=float(cap["ss"][0][6]))
        return out
    finally:
        os.chdir(cwd)
        fm_mod.ForwardModel_0.CIRSrad = o_cirs
        ms_mod.scloud11wave_core = o_core
        fm_mod.ForwardModel_0.calculate_vertical_cia_opacity = o_cia
        fm_mod.calc_singlescatt_plane_spectrum = o_ss


def main():
    ans = import_reference()
    sp_mod = sys.modules["archnemesis.Spectroscopy_0"]
    fm_mod = sys.modules["archnemesis.ForwardModel_0"]
    ms_mod = importlib.import_module("archnemesis.Multiple_Scattering_Core")
    src = os.path.join(REFERENCE_ROOT, "tests", "files", "Jupiter_CIRS_angled_thermal_emission_scattering")
    work = tempfile.mkdtemp(prefix="ansfm_c4_lbl_")
    try:
        for f in os.listdir(src):
            shutil.copy(os.path.join(src, f), os.path.join(work, f))
            os.chmod(os.path.join(work, f), 0o644)
        _write_tables(sp_mod, work)
        out = _run(ans, fm_mod, ms_mod, work, 1)
        ss = _run(ans, fm_mod, ms_mod, work, 3)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert np.array_equal(ss["WAVE"], out["WAVE"]) and np.array_equal(ss["K"], out["K"])
    # the single-scattering run: its own keys, and under ss_ what differs from the multiple-scattering run (the layers, their
    # opacities and the geometry are the same: kept once)
    for k_, v in ss.items():
        if k_.startswith("ss_"):
            out[k_] = v
        elif not (k_ in out and np.array_equal(np.asarray(v), np.asarray(out[k_]))):
            out["ss_" + k_] = v
    fn = os.path.join(OUT, "c4_lbl_scatter.npz")
    np.savez_compressed(fn, **out)
    print("wrote", fn, os.path.getsize(fn) / 1e6, "MB")
    for k_, v in out.items():
        if hasattr(v, "shape"):
            print(k_, v.shape)


if __name__ == "__main__":
    main()
