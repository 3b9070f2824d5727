"""Host-side mirror of the reference's ForwardModel_0 surface for the hot path.

`make_gpu_forward_model(ForwardModel_0)` returns a subclass of the reference's own class
(ForwardModel_0.py:87) whose `CIRSrad` (ForwardModel_0.py:4376-4511) runs on the MI355X through
libansfm.so for the supported cases (ILBL = K_TABLES, LINE_BY_LINE_TABLES or LINE_BY_LINE_RUNTIME with line data in
SpectroscopyX, IMOD = THERMAL_EMISSION, no layer emissions, with or without analytic gradients) and whose `jacobian_nemesis` fan-out can batch the independent forward models.
Everything else (subprofretg, calc_path, conv, ...) is the reference's own host code.

`CIRSradGPU` is the mixin with the seam itself; it only needs the `*X` attributes CIRSrad reads
(SpectroscopyX, LayerX, PathX, AtmosphereX, SurfaceX, MeasurementX, ScatterX, StellarX, CIAX,
EmissionsX), so tests drive it with plain namespaces rebuilt from the C1 golden fixture.
"""
import hashlib
import os
import sys

import numpy as np

from .engine import AnsfmEngine

# IntEnum / IntFlag values of the reference (archnemesis/enum/*.py) kept as plain ints at the seam
ILBL_K_TABLES = 0                      # SpectralCalculationModeEnum.K_TABLES
ILBL_LBL_TABLES = 2                    # SpectralCalculationModeEnum.LINE_BY_LINE_TABLES
ILBL_LBL_RUNTIME = 1                   # SpectralCalculationModeEnum.LINE_BY_LINE_RUNTIME
IMOD_THERMAL_EMISSION = 64             # PathCalcEnum.THERMAL_EMISSION
IMOD_MULTIPLE_SCATTERING = 256
IMOD_DOWNWARD_FLUX = 16
IMOD_SINGLE_SCATTERING_PLANE_PARALLEL = 1024
IMOD_ABSORBTION = 4096
IFORM_FLUXRATIO = 1                    # SpectraUnitEnum.FluxRatio
IFORM_TRANSIT_DEPTH = 2                # SpectraUnitEnum.TransitDepth
IFORM_ATMOSPHERIC_TRANSMISSION = 4     # SpectraUnitEnum.Atmospheric_transmission
IFORM_INTEGRATED_RADIANCE = 6          # SpectraUnitEnum.Integrated_radiance
ATM_TO_PASCAL = 101325.0               # ForwardModel_0.py:61
SQ_CM_TO_SQ_METER = 1.0e-4             # ForwardModel_0.py:66

_ENGINES = {}


def _planck(ispace, wave, temp):
    """planck (ForwardModel_0.py:6183-6227): W cm-2 sr-1 (cm-1)-1 for wavenumbers (ISPACE 0), W cm-2 sr-1 um-1 for
    wavelengths in micron (ISPACE 1); c1 = 1.1911e-12, c2 = 1.439 as there."""
    wave = np.asarray(wave, dtype=np.float64)
    c1, c2 = 1.1911e-12, 1.439
    if int(ispace) == 0:
        y, a = wave, c1 * wave ** 3
    else:
        y = 1.0e4 / wave
        a = c1 * y ** 5 / 1.0e4
    return a / (np.exp(c2 * y / temp) - 1.0)


def get_engine(device=0):
    """One engine (ctx) per GPU per process."""
    if device not in _ENGINES:
        _ENGINES[device] = AnsfmEngine(device)
    return _ENGINES[device]


# What the adapter does with a case the GPU path does not cover (another IMOD, a line shape that is not built, an unsorted
# calculation grid, a non-binary table ...): by default the call goes to the reference's own function -- the reference's
# code in the reference's process, never a CPU re-implementation of this package -- and is counted in DELEGATED; with
# set_strict(True) it raises NotImplementedError instead, so a run can prove that nothing left the GPU path.
STRICT = False
DELEGATED = {}


def set_strict(on=True):
    global STRICT
    STRICT = bool(on)


def _delegate(what):
    if STRICT:
        raise NotImplementedError("ansfm (strict): %s is outside the GPU path and delegation to the reference is off" % what)
    if what not in DELEGATED:            # said once per kind of case, counted every time (DELEGATED)
        import warnings
        warnings.warn("ansfm: %s is outside the GPU path; handed to the reference's own CPU implementation "
                      "(set_strict(True) turns this into an error)" % what, RuntimeWarning, stacklevel=3)
    DELEGATED[what] = DELEGATED.get(what, 0) + 1


NOTES = {}


def _note(what):
    """Something the adapter does differently from the reference on purpose (not a delegation: the work stays on the GPU
    path), said once as a RuntimeWarning and counted in NOTES -- e.g. NCores > 1 without joblib workers."""
    if what not in NOTES:
        import warnings
        warnings.warn("ansfm: " + what, RuntimeWarning, stacklevel=3)
    NOTES[what] = NOTES.get(what, 0) + 1


ROUTES = {}


def _route(what):
    """A GPU route that a run may want to see it took (counted in ROUTES, not announced): e.g. CIRSrad on the line source."""
    ROUTES[what] = ROUTES.get(what, 0) + 1


def summary():
    """What left the GPU path (DELEGATED: case -> count), what was done differently on purpose (NOTES) and which of the
    counted GPU routes ran (ROUTES) since the process started or `reset_summary()`; `install_all()` returns the same
    object, so a caller can print it after a retrieval."""
    return {"delegated": dict(DELEGATED), "notes": dict(NOTES), "routes": dict(ROUTES), "strict": STRICT}


def reset_summary():
    DELEGATED.clear()
    NOTES.clear()
    ROUTES.clear()


class KtaTableOnDevice:
    """Stand-in for Spectroscopy.K when the k-table is taken from the .kta files straight into HBM
    (install_gpu_table_reader): knows the files, the wavenumber range and the shape the array would have.  Code that
    really needs the numbers on the host (a CPU path of the reference) gets them through __array__, read by the
    reference's own read_ktable -- slowly, once."""

    def __init__(self, paths, wavemin, wavemax, shape, reader, ext=".kta", kindex=12):
        self.ext, self._kindex = ext, kindex      # ".lta": read_lbltable returns k as its 9th item
        self.paths = [str(p) for p in paths]
        self.wavemin, self.wavemax = float(wavemin), float(wavemax)
        self.shape = tuple(int(x) for x in shape)
        self.ndim = len(self.shape)
        self.dtype = np.dtype(np.float64)
        self._reader = reader
        self._host = None
        st = []
        for p in self.paths:
            q = p if p.endswith(ext) else p + ext
            s = os.stat(q)
            st.append((q, s.st_size, s.st_mtime_ns))
        self.fingerprint = hashlib.blake2b(repr((st, self.wavemin, self.wavemax, self.shape)).encode(), digest_size=16).hexdigest()

    def __array__(self, dtype=None, copy=None):
        if self._host is None:
            k = np.zeros(self.shape)
            for i, p in enumerate(self.paths):
                k[..., i] = self._reader(p, self.wavemin, self.wavemax)[self._kindex]
            self._host = k
        return self._host if dtype is None else self._host.astype(dtype, copy=False)

    def __deepcopy__(self, memo):
        return self                      # immutable description of files; nemesisfm deep-copies Spectroscopy per call


def _table_fingerprint(S):
    """Cheap content fingerprint of the k-table held by a Spectroscopy object.  nemesisfm
    deep-copies Spectroscopy and re-reads the tables for every forward model
    (ForwardModel_0.py:480-482); the table in HBM is re-used when nothing changed."""
    K = S.K
    h = hashlib.blake2b(digest_size=16)
    if isinstance(K, KtaTableOnDevice):
        h.update(K.fingerprint.encode())
        for a in (S.WAVE, S.PRESS, S.TEMP, S.DELG):
            h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        return h.hexdigest()
    h.update(np.asarray(K.shape, dtype=np.int64).tobytes())
    h.update(str(int(S.ILBL)).encode())
    flat = K.reshape(-1)
    step = max(1, flat.size // 8192)
    h.update(np.ascontiguousarray(flat[::step]).tobytes())
    for a in (S.WAVE, S.PRESS, S.TEMP, S.DELG):
        h.update(str(getattr(a, "dtype", "")).encode())          # float32 grids select float32 semantics
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


class CIRSradGPU:
    """Mixin: CIRSrad on the GPU.  Put it in front of the reference class in the MRO."""

    ansfm_device = 0
    ansfm_keep_side_products = True   # fill LayerX.TAUGAS / TAUTOT like the reference (:3925, :3997)
    # Opt-in: CIRSrad(return_grad=True) computes the gas-amount gradients only of the gases the last subprofretg() mapped
    # to the state vector (non-zero xmap rows: what nemesisfmg's own `incpar` keeps for map2pro, :699-702); the other gases'
    # parameters of dSPECOUT then hold their continuum part only.  dSPECONV is unchanged, the gradient merge is not.
    ansfm_select_gradient_gases = False

    def subprofretg(self, *a, **k):
        xmap = super().subprofretg(*a, **k)
        self._ansfm_xmap = xmap
        return xmap

    # ---- what is supported -----------------------------------------------------------------------
    def _ansfm_supported(self, return_grad):
        S = self.SpectroscopyX
        if S.NGAS > 0 and int(S.ILBL) == ILBL_LBL_RUNTIME:
            if self._ansfm_line_source()[0] is None:      # the cases of the line source that are built, nothing else
                return False
        elif S.NGAS <= 0 or int(S.ILBL) not in (ILBL_K_TABLES, ILBL_LBL_TABLES) or S.K is None:
            return False
        if return_grad and (self.AtmosphereX.NVMR + 2 + self.ScatterX.NDUST > 256 or S.NGAS > 31):
            return False                   # kMaxPar of the gradient kernels' slot table; one mask bit per gas
        if getattr(self, "EmissionsX", None) is not None:
            return False
        imod = np.unique(np.asarray(self.PathX.IMOD).astype(int))
        if imod.size != 1:
            return False
        imod = int(imod[0])
        # dispatch order of CIRSrad :4478-4501: transmission / absorption come before thermal emission, thermal emission
        # before single scattering, the downward-flux variant before plain multiple scattering
        if self._ansfm_transmission_branch(imod):
            return True
        if imod & IMOD_ABSORBTION:
            return False           # calculate_absorption_spectrum (:4133) lacks `self` in the reference: never callable
        if imod & IMOD_THERMAL_EMISSION:
            return True
        # the scattering branches: k-tables or LBL tables (G = 1), without gradients -- the reference has none there either
        if imod & IMOD_SINGLE_SCATTERING_PLANE_PARALLEL:
            return not return_grad
        if self._ansfm_scatter_branch(imod):
            return not return_grad
        return False

    # ---- runtime line-by-line (ILBL = 1): the line source and the state of a call -------------------------------------
    def _ansfm_line_source(self):
        """(LineSource, None) when the runtime line-by-line opacity of this model is built on the device, else (None, why):
        SpectroscopyX carries LINE_DATA / LINE_DATA_PARAMS, every line shape is built, the bins pass the pseudo-continuum
        entry's tests, the spectral axis is wavenumber."""
        from . import line_source as lsrc
        S = self.SpectroscopyX
        ld, prm = getattr(S, "LINE_DATA", None), getattr(S, "LINE_DATA_PARAMS", None)
        if not ld or not prm or len(ld) != S.NGAS or len(prm) != S.NGAS:
            return None, "no LINE_DATA / LINE_DATA_PARAMS for every gas"
        if int(getattr(S, "ISPACE", 0)) != 0:
            return None, "a wavelength grid"
        try:
            src = lsrc.LineSource.from_spectroscopy(S)
        except (AttributeError, TypeError, ValueError, IndexError) as e:
            return None, "line data this adapter cannot read (%s)" % e
        why = src.unsupported()
        return (None, why) if why else (src, None)

    def _ansfm_line_state(self, eng, src, return_grad):
        """amb_frac as :3822-3827, the q ratios from partition_fn_data at t_ref / t_cont against T (and T + 5 K), the distinct
        k-rows of the layers -> the engine's state for the call that follows"""
        from . import line_source as lsrc
        S, L, A = self.SpectroscopyX, self.LayerX, self.AtmosphereX
        amb = lsrc.ambient_fractions(L.PP, L.PRESS, A.ID, S.ID)
        if src.M != 2:
            raise ValueError("ILBL = 1 in CIRSrad: amb_frac has one ambient gas (ForwardModel_0.py:3823), the line data %d" % (src.M - 1))
        st = lsrc.pack_line_state(src, np.asarray(L.PRESS, dtype=np.float64) / lsrc.ATM_TO_PASCAL, L.TEMP, lsrc.mix_fractions(amb),
                                  grad=return_grad)
        eng.set_line_state(st)
        return st

    @staticmethod
    def _ansfm_transmission_branch(imod):
        """the first test of CIRSrad's dispatch (:4478-4483): none of the four flags -> exp(-tau)"""
        return not (imod & (IMOD_ABSORBTION | IMOD_THERMAL_EMISSION | IMOD_MULTIPLE_SCATTERING |
                            IMOD_SINGLE_SCATTERING_PLANE_PARALLEL))

    @staticmethod
    def _ansfm_scatter_branch(imod):
        return bool(imod & IMOD_MULTIPLE_SCATTERING) and not (
            imod & (IMOD_ABSORBTION | IMOD_THERMAL_EMISSION | IMOD_SINGLE_SCATTERING_PLANE_PARALLEL | IMOD_DOWNWARD_FLUX))

    # ---- continuum opacities: the reference's own host routines when present ---------------------
    def _ansfm_continuum(self, return_grad=False):
        """Returns TAUCIA, TAUDUST, TAURAY (NWAVE,NLAY) and, for return_grad, dTAUCON (NWAVE,NPAR,NLAY)
        assembled exactly as calculate_layer_opacity does (:3916-3981)."""
        S, L = self.SpectroscopyX, self.LayerX
        dTAUCON = None
        if hasattr(self, "calculate_vertical_cia_opacity"):
            A, Sc = self.AtmosphereX, self.ScatterX
            TAUCIA, dTAUCIA = self.calculate_vertical_cia_opacity(return_grad)   # :3938 (sets LayerX.TAUCIA)
            TAURAY, dTAURAY = self.calc_tau_rayleigh(MakePlot=False)              # :3952
            L.TAURAY = TAURAY
            TAUDUST1, TAUCLSCAT, dTAUDUST1, dTAUCLSCAT = self.calc_tau_dust()     # :3963
            TAUDUST1 = np.clip(np.nan_to_num(TAUDUST1), 0, 1e20)                 # :3966
            TAUDUST = np.sum(TAUDUST1, 2)
            L.TAUDUST = TAUDUST
            L.TAUSCAT = np.sum(TAUCLSCAT, 2)
            L.TAUCLSCAT = TAUCLSCAT
            if return_grad:
                dTAUCON = np.zeros((S.NWAVE, A.NVMR + 2 + Sc.NDUST, L.NLAY))
                if dTAUCIA is not None:                                           # :3940-3942
                    # d TAUCIA / d amount of every gas: per unit column, with the gas axis ahead of the layer axis
                    dTAUCON[:, 0:A.NVMR, :] += np.moveaxis(dTAUCIA[:, :, 0:A.NVMR], 2, 1) / np.asarray(L.TOTAM)[None, None, :]
                    dTAUCON[:, A.NVMR, :] += dTAUCIA[:, :, A.NVMR]
                if dTAURAY is not None:                                           # :3955-3957
                    for i in range(A.NVMR):
                        dTAUCON[:, i, :] += dTAURAY[:, :]
                for i in range(Sc.NDUST):                                         # :3978-3980
                    dTAUCON[:, A.NVMR + 1 + i, :] += dTAUDUST1[:, :, i]
        else:  # standalone: continuum arrays were provided on LayerX
            dTAUCON = getattr(L, "dTAUCON", None) if return_grad else None
            z = np.zeros((S.NWAVE, L.NLAY))
            TAUCIA = getattr(L, "TAUCIA", None)
            TAUCIA = z if TAUCIA is None else TAUCIA
            TAURAY = getattr(L, "TAURAY", None)
            TAURAY = z if TAURAY is None else TAURAY
            TAUDUST = getattr(L, "TAUDUST", None)
            TAUDUST = z if TAUDUST is None else TAUDUST
        return TAUCIA, TAUDUST, TAURAY, dTAUCON

    @staticmethod
    def _ansfm_total_opacity(TAUGAS, TAUCIA, TAUDUST, TAURAY):
        """LayerX.TAUTOT (NWAVE, NG, NLAY): the continuum terms joined to every g-ordinate in the order of :3989."""
        out = TAUGAS.copy()
        for cont in (TAUCIA, TAUDUST, TAURAY):
            out += cont[:, None, :]
        return out

    def _ansfm_units_and_surface(self):
        """xfac and EMISSIVITY exactly as calculate_thermal_emission_spectrum prepares them
        (ForwardModel_0.py:4157-4189).  REFLECTANCE is identically zero there (:4208-4213), so the
        solar-reflection term vanishes and SOLFLUX is not needed."""
        import scipy.interpolate
        S = self.SpectroscopyX
        xfac = None
        if int(self.MeasurementX.IFORM) == IFORM_FLUXRATIO:
            xfac = np.ones(S.NWAVE) * np.pi * 4. * np.pi * ((self.AtmosphereX.RADIUS) * 1.0e2) ** 2.
            self.StellarX.calc_solar_flux()
            f = scipy.interpolate.interp1d(self.StellarX.WAVE, self.StellarX.SOLFLUX)
            xfac = xfac / f(S.WAVE)
        if self.SurfaceX.TSURF > 0.0:
            f = scipy.interpolate.interp1d(self.SurfaceX.VEM, self.SurfaceX.EMISSIVITY)
            emissivity = f(S.WAVE)
        else:
            emissivity = None
        return xfac, emissivity

    def _ansfm_upload_table(self, eng):
        S = self.SpectroscopyX
        if int(S.ILBL) == ILBL_LBL_RUNTIME:           # the line source, once per fingerprint of the line data and parameters
            src = self._ansfm_line_source()[0]
            fp = "lines:" + src.fingerprint()
            if getattr(eng, "_table_fp", None) != fp:
                eng.upload_line_source(src)
                eng._table_fp = fp
            return src
        fp = _table_fingerprint(S)
        if getattr(eng, "_table_fp", None) != fp:
            if isinstance(S.K, KtaTableOnDevice):   # .kta / .lta files -> HBM without a host array (install_gpu_table_reader)
                up = eng.upload_lbltable_files if S.K.ext == ".lta" else eng.upload_ktable_files
                WAVE = up(S.K.paths, S.K.wavemin, S.K.wavemax)[0]
                if WAVE.shape != np.shape(S.WAVE) or not np.array_equal(WAVE, np.asarray(S.WAVE, dtype=np.float64)):
                    raise ValueError("the .kta files no longer give the wavenumber grid Spectroscopy.WAVE holds")
            elif int(S.ILBL) == ILBL_LBL_TABLES:      # K (NWAVE,NP,|NT|,NGAS); TEMP (NP,|NT|) when NT < 0
                eng.upload_lbltable(np.ascontiguousarray(S.K, dtype=np.float64), S.PRESS, S.TEMP, S.WAVE)
            else:
                eng.upload_ktable(np.ascontiguousarray(S.K, dtype=np.float64), S.PRESS, S.TEMP, S.WAVE, S.DELG)
            eng._table_fp = fp

    def _ansfm_layer_inputs(self):
        S, L, A = self.SpectroscopyX, self.LayerX, self.AtmosphereX
        f_gas = np.zeros((S.NGAS, L.NLAY))
        for i in range(S.NGAS):
            IGAS = A.locate_gas(S.ID[i], S.ISO[i])
            f_gas[i, :] = L.AMOUNT[:, IGAS] * SQ_CM_TO_SQ_METER             # :3861
        return f_gas

    # ---- single-scattering branch: host preparation of :4251-4336 for what has no g axis ---------------------------
    def _ansfm_cirsrad_singlescatt(self, eng=None, taucont=None, TAURAY=None, f_gas=None):
        """calculate_single_scattering_plane_parallel_spectrum (:4251-4336): scattering angle, phase functions of the aerosols
        and of Rayleigh scattering, their opacity-weighted mean per layer, solar flux, units, emissivity and BRDF on the host;
        OMEGA and the layer loop (calc_singlescatt_plane_spectrum :6509) on the device.  -> SPECOUT (NWAVE, NPATH); without an
        engine, the prepared arguments."""
        import scipy.interpolate
        S, L, P, Sc, Su, M = self.SpectroscopyX, self.LayerX, self.PathX, self.ScatterX, self.SurfaceX, self.MeasurementX
        WAVE = np.asarray(S.WAVE, dtype=np.float64)
        W, ND = WAVE.size, int(Sc.NDUST)
        sol, emi, azi = (np.asarray(a, dtype=np.float64) for a in (P.SOL_ANG, P.EMISS_ANG, P.AZI_ANG))
        rad = np.pi / 180.
        calpha = np.sin(sol * rad) * np.sin(emi * rad) * np.cos(azi * rad - np.pi) - np.cos(emi * rad) * np.cos(sol * rad)   # :4267
        alpha = np.arccos(calpha) / np.pi * 180.
        pf = np.zeros((W, len(sol), ND + 1))                                     # :4271-4274
        pf[:, :, 0:ND] = Sc.calc_phase(alpha, WAVE)
        pf[:, :, ND] = Sc.calc_phase_ray(alpha)
        TAUSCAT, TAUCLSCAT = L.TAUSCAT, L.TAUCLSCAT
        tsca = TAURAY + TAUSCAT
        # layer-mean phase function of every path: sum_c P_c(alpha) tau_c / (TAURAY + TAUSCAT) where that is > 0 (:4314-4322)
        num = np.einsum("wpc,wlc->pwl", pf[:, :, 0:ND], TAUCLSCAT) + pf[:, :, ND].T[:, :, None] * TAURAY[None, :, :]
        phase = np.where(num > 0, num / np.where(num > 0, tsca[None], 1.0), num)
        if self.StellarX.SOLEXIST is True:                                       # :4286-4290
            self.StellarX.calc_solar_flux()
            solar = np.interp(WAVE, self.StellarX.WAVE, self.StellarX.SOLFLUX)
        else:
            solar = np.zeros(W)
        xfac = np.ones(W)
        if int(M.IFORM) == IFORM_FLUXRATIO:                                      # :4293-4298 (the power spectrum on VCONV)
            xfac *= np.pi * 4. * np.pi * ((self.AtmosphereX.RADIUS) * 1.0e2) ** 2.
            xfac = xfac / scipy.interpolate.interp1d(self.StellarX.VCONV, self.StellarX.SOLSPEC)(WAVE)
        if Su.TSURF > 0.0:
            emissivity = scipy.interpolate.interp1d(Su.VEM, Su.EMISSIVITY)(WAVE)
        else:
            emissivity = np.zeros(W)
        if int(Su.LOWBC) != 0:                                                   # :4308-4311 (0 = THERMAL)
            BRDF = Su.calc_BRDF(WAVE, P.SOL_ANG, P.EMISS_ANG, P.AZI_ANG)
        else:
            BRDF = np.zeros((W, len(sol)))
        NPATH = len(sol)
        args = dict(ISPACE=int(M.ISPACE), lp=np.array(L.PRESS, dtype=np.float64), lt=np.array(L.TEMP, dtype=np.float64), f_gas=f_gas,
                    taucont=np.asarray(taucont, dtype=np.float64), tausca=tsca, phase=phase,
                    NLAYIN=np.asarray(P.NLAYIN, dtype=np.int32).reshape(NPATH), LAYINC=np.asarray(P.LAYINC, dtype=np.int32).reshape(-1, NPATH),
                    SCALE=np.asarray(P.SCALE, dtype=np.float64).reshape(-1, NPATH),
                    EMTEMP=np.asarray(P.EMTEMP, dtype=np.float64).reshape(-1, NPATH), TSURF=float(Su.TSURF), emissivity=emissivity,
                    BRDF=np.asarray(BRDF, dtype=np.float64).reshape(W, NPATH), solar=solar, SOL_ANG=sol.reshape(NPATH),
                    EMISS_ANG=emi.reshape(NPATH), xfac=xfac)
        if eng is None:                  # the staged Jacobian route keeps the arguments and batches the call
            return args
        return self._ansfm_singlescatt_call(eng, args)

    @staticmethod
    def _ansfm_singlescatt_call(eng, a):
        return eng.cirsrad_ck_singlescatt(a["ISPACE"], a["lp"], a["lt"], a["f_gas"], a["taucont"], a["tausca"], a["phase"], a["NLAYIN"],
                                          a["LAYINC"], a["SCALE"], a["EMTEMP"], a["TSURF"], a["emissivity"], a["BRDF"], a["solar"],
                                          a["SOL_ANG"], a["EMISS_ANG"], xfac=a["xfac"])

    # ---- scattering branch: host preparation of scloud11wave (:5018-5165) for what has no g axis ----------------
    def _ansfm_cirsrad_scatter(self, eng, TAUCIA, TAUDUST, TAURAY, f_gas):
        """calculate_multiple_scattering_spectrum (:4343-4374) + scloud11wave (:5018-5165): the boundary vectors, phase
        functions and aerosol fractions are small host arrays prepared as the reference does; the gas opacities, TAUTOT,
        OMEGA and BB are formed on the device (ansfm_cirsrad_ck_scatter).  -> SPECOUT (NWAVE, NPATH)."""
        import scipy.interpolate
        S, L, P, Sc, Su, M = self.SpectroscopyX, self.LayerX, self.PathX, self.ScatterX, self.SurfaceX, self.MeasurementX
        WAVE = np.asarray(S.WAVE, dtype=np.float64)
        W, ISPACE = WAVE.size, int(M.ISPACE)
        solar = np.zeros(W)
        if self.StellarX.SOLEXIST:                                               # :4353-4357
            self.StellarX.calc_solar_flux()
            solar[:] = scipy.interpolate.interp1d(self.StellarX.WAVE, self.StellarX.SOLFLUX)(WAVE)
        # (the reference works xfac out here, :4359-4368, and never applies it to this branch's spectrum: nor is it here)
        NMU, NDUST = int(Sc.NMU), int(Sc.NDUST)
        RADGROUND = np.zeros((W, NMU))
        if Su.GASGIANT or (Su.TSURF <= 0.0):                                     # :5082-5089
            RADGROUND[:, :] = _planck(ISPACE, WAVE, L.TEMP[0])[:, None]
        else:
            emis = scipy.interpolate.interp1d(Su.VEM, Su.EMISSIVITY)(WAVE)
            RADGROUND[:, :] = (_planck(ISPACE, WAVE, Su.TSURF) * emis)[:, None]
        if (not Su.GASGIANT) and int(Su.LOWBC) != 0:                             # :5091-5094 (0 = THERMAL)
            BRDF = self.calc_brdf_matrix(WAVEC=WAVE, Surface=Su, Scatter=Sc)
        else:
            BRDF = np.zeros((W, NMU, NMU, int(Sc.NF) + 1))
        TAUSCAT, TAUCLSCAT = L.TAUSCAT, L.TAUCLSCAT
        FRAC = np.zeros((W, L.NLAY, NDUST))                                      # :5106-5114
        pos = TAUSCAT > 0.0
        FRAC[pos] = TAUCLSCAT[pos] / TAUSCAT[pos][:, None]
        FRAC = np.ascontiguousarray(np.transpose(FRAC, (0, 2, 1)))
        THETA = np.asarray(Sc.THETA, dtype=np.float64)
        PHASE = np.zeros((NDUST, W, 2, THETA.size))                              # :5125-5137
        if int(Sc.IMIE) == 0:                                                    # Henyey-Greenstein: f, g1, g2
            for i in range(NDUST):
                PHASE[i, :, 0, -1] = np.interp(WAVE, Sc.WAVE, Sc.F.T[i])
                PHASE[i, :, 0, -2] = np.interp(WAVE, Sc.WAVE, Sc.G1.T[i])
                PHASE[i, :, 0, -3] = np.interp(WAVE, Sc.WAVE, Sc.G2.T[i])
        else:
            PHASE[:, :, 0, :] = np.transpose(Sc.calc_phase(THETA, WAVE), (2, 0, 1))
        PHASE[:, :, 1, :] = np.cos(THETA * np.pi / 180)
        args = dict(ISPACE=ISPACE, lp=np.array(L.PRESS, dtype=np.float64), lt=np.array(L.TEMP, dtype=np.float64), f_gas=f_gas,
                    TAUCIA=np.asarray(TAUCIA, dtype=np.float64), TAUDUST=np.asarray(TAUDUST, dtype=np.float64),
                    TAURAY=np.asarray(TAURAY, dtype=np.float64), TAUSCAT=np.asarray(TAUSCAT, dtype=np.float64),
                    PHASE=np.ascontiguousarray(PHASE[:, :, :, ::-1]), FRAC=FRAC, RADGROUND=RADGROUND,
                    SOL_ANG=np.array(P.SOL_ANG, dtype=np.float64).reshape(-1), EMISS_ANG=np.array(P.EMISS_ANG, dtype=np.float64).reshape(-1),
                    AZI_ANG=np.array(P.AZI_ANG, dtype=np.float64).reshape(-1), solar=solar, LOWBC=int(Su.LOWBC), BRDF=BRDF,
                    MU=np.array(Sc.MU, dtype=np.float64), WTMU=np.array(Sc.WTMU, dtype=np.float64), NF=int(Sc.NF), NPHI=int(Sc.NPHI),
                    IRAY=int(Sc.IRAY), IMIE=int(Sc.IMIE))
        if eng is None:                  # the staged Jacobian route keeps the arguments and batches the call
            return args
        return self._ansfm_scatter_call(eng, args)

    @staticmethod
    def _ansfm_scatter_call(eng, a):
        return eng.cirsrad_ck_scatter(a["ISPACE"], a["lp"], a["lt"], a["f_gas"], a["TAUCIA"], a["TAUDUST"], a["TAURAY"], a["TAUSCAT"],
                                      a["PHASE"], a["FRAC"], a["RADGROUND"], a["SOL_ANG"], a["EMISS_ANG"], a["AZI_ANG"], a["solar"],
                                      a["LOWBC"], a["BRDF"], a["MU"], a["WTMU"], a["NF"], a["NPHI"], a["IRAY"], a["IMIE"])

    # ---- the seam ---------------------------------------------------------------------------------
    def CIRSrad(self, return_grad=False):
        if not self._ansfm_supported(return_grad):
            S = self.SpectroscopyX
            why = self._ansfm_line_source()[1] if (S.NGAS > 0 and int(S.ILBL) == ILBL_LBL_RUNTIME) else None
            _delegate("CIRSrad on runtime line-by-line opacities with " + why if why else "CIRSrad case (IMOD / ILBL / emissions)")
            base = super()
            if hasattr(base, "CIRSrad"):
                return base.CIRSrad(return_grad)      # the reference's own implementation, in its process
            raise NotImplementedError("CIRSrad: only ILBL=K_TABLES, IMOD=THERMAL_EMISSION run on the GPU so far")
        eng = get_engine(self.ansfm_device)
        S, L, P = self.SpectroscopyX, self.LayerX, self.PathX
        src = self._ansfm_upload_table(eng)
        if src is not None:                           # ILBL = 1: the k-rows of this call's layers
            self._ansfm_line_state(eng, src, return_grad)
            _route("CIRSrad on runtime line-by-line opacities (ILBL = 1, line source in HBM)")
        TAUCIA, TAUDUST, TAURAY, dTAUCON = self._ansfm_continuum(return_grad)
        taucont = TAUCIA + TAUDUST + TAURAY                                  # :3989 (g-independent part)
        f_gas = self._ansfm_layer_inputs()
        if self._ansfm_scatter_branch(int(np.unique(np.asarray(P.IMOD).astype(int))[0])):
            SPECOUT = self._ansfm_cirsrad_scatter(eng, TAUCIA, TAUDUST, TAURAY, f_gas)
            if self.ansfm_keep_side_products:
                L.TAUGAS = eng.get_taugas(L.NLAY, 0)                         # :3925
                L.TAUTOT = self._ansfm_total_opacity(L.TAUGAS, TAUCIA, TAUDUST, TAURAY)
            return SPECOUT
        imod0 = int(np.unique(np.asarray(P.IMOD).astype(int))[0])
        if self._ansfm_transmission_branch(imod0):
            import scipy.interpolate
            xf = None
            if int(self.MeasurementX.IFORM) == IFORM_ATMOSPHERIC_TRANSMISSION:   # :4119-4127: times the solar flux
                self.StellarX.calc_solar_flux()
                xf = scipy.interpolate.interp1d(self.StellarX.WAVE, self.StellarX.SOLFLUX)(S.WAVE)
            NPATH = np.asarray(P.LAYINC).shape[1]
            geom = (np.asarray(P.NLAYIN, dtype=np.int32).reshape(NPATH), np.asarray(P.LAYINC, dtype=np.int32).reshape(-1, NPATH),
                    np.asarray(P.SCALE, dtype=np.float64).reshape(-1, NPATH))
            lp, lt = np.asarray(L.PRESS, dtype=np.float64), np.asarray(L.TEMP, dtype=np.float64)
            if return_grad:                                                  # :4128-4131, then :4504-4508
                A = self.AtmosphereX
                NVMR = int(A.NVMR)
                NPAR = NVMR + 2 + int(self.ScatterX.NDUST)
                igas_map = np.array([A.locate_gas(S.ID[i], S.ISO[i]) for i in range(S.NGAS)], dtype=np.int32)
                SPECOUT, dSPECOUT = eng.cirsradg_ck_transmission(lp, lt, f_gas, taucont, dTAUCON, NVMR, NPAR, igas_map, *geom,
                                                                 xfac=xf)
            else:
                SPECOUT = eng.cirsrad_ck_transmission(lp, lt, f_gas, taucont, *geom, xfac=xf)
            if self.ansfm_keep_side_products:
                L.TAUGAS = eng.get_taugas(L.NLAY, 0)
                L.TAUTOT = self._ansfm_total_opacity(L.TAUGAS, TAUCIA, TAUDUST, TAURAY)
            if return_grad:
                return SPECOUT, dSPECOUT, np.zeros_like(SPECOUT)             # dTSURF: zeros through the g-quadrature
            return SPECOUT
        if (imod0 & IMOD_SINGLE_SCATTERING_PLANE_PARALLEL) and not (imod0 & IMOD_THERMAL_EMISSION):   # dispatch order :4487-4493
            SPECOUT = self._ansfm_cirsrad_singlescatt(eng, taucont, TAURAY, f_gas)
            if self.ansfm_keep_side_products:
                L.TAUGAS = eng.get_taugas(L.NLAY, 0)
                L.TAUTOT = self._ansfm_total_opacity(L.TAUGAS, TAUCIA, TAUDUST, TAURAY)
            return SPECOUT
        xfac, emissivity = self._ansfm_units_and_surface()
        NPATH = int(P.NPATH) if hasattr(P, "NPATH") else np.asarray(P.LAYINC).shape[1]
        LAYINC = np.asarray(P.LAYINC, dtype=np.int32).reshape(-1, NPATH)
        NLAYIN = np.asarray(P.NLAYIN, dtype=np.int32).reshape(NPATH)
        SCALE = np.asarray(P.SCALE, dtype=np.float64).reshape(-1, NPATH)
        EMTEMP = np.asarray(P.EMTEMP, dtype=np.float64).reshape(-1, NPATH)
        if return_grad:
            A = self.AtmosphereX
            NVMR = int(A.NVMR)
            NPAR = NVMR + 2 + int(self.ScatterX.NDUST)
            igas_map = np.array([A.locate_gas(S.ID[i], S.ISO[i]) for i in range(S.NGAS)], dtype=np.int32)
            xm = getattr(self, "_ansfm_xmap", None) if self.ansfm_select_gradient_gases else None
            selected = xm is not None and np.ndim(xm) == 3 and np.shape(xm)[1] == NPAR and hasattr(eng, "set_gradient_gases")
            if selected:
                used = np.any(np.asarray(xm) != 0.0, axis=(0, 2))
                eng.set_gradient_gases([i for i in range(S.NGAS) if used[igas_map[i]]], temperature=bool(used[NVMR]))
            try:
                SPECOUT, dSPECOUT, dTSURF = eng.cirsradg_ck_thermal(
                    int(self.MeasurementX.ISPACE), np.asarray(L.PRESS, dtype=np.float64),
                    np.asarray(L.TEMP, dtype=np.float64), f_gas, taucont, dTAUCON, NVMR, NPAR, igas_map, NLAYIN, LAYINC,
                    SCALE, EMTEMP, float(self.SurfaceX.TSURF), EMISSIVITY=emissivity, xfac=xfac)
            finally:
                if selected:
                    eng.set_gradient_gases(None)
        else:
            SPECOUT = eng.cirsrad_ck_thermal(
                int(self.MeasurementX.ISPACE), np.asarray(L.PRESS, dtype=np.float64),
                np.asarray(L.TEMP, dtype=np.float64), f_gas, taucont, NLAYIN, LAYINC, SCALE, EMTEMP,
                float(self.SurfaceX.TSURF), EMISSIVITY=emissivity,
                SOL_ANG=np.asarray(P.SOL_ANG, dtype=np.float64).reshape(NPATH),
                EMISS_ANG=np.asarray(P.EMISS_ANG, dtype=np.float64).reshape(NPATH), xfac=xfac)
        if self.ansfm_keep_side_products:
            L.TAUGAS = eng.get_taugas(L.NLAY, 0)                             # :3925
            L.TAUTOT = self._ansfm_total_opacity(L.TAUGAS, TAUCIA, TAUDUST, TAURAY)
        if return_grad:
            return SPECOUT, dSPECOUT, dTSURF          # (NWAVE,NPATH), (NWAVE,NPAR,NLAYINmax,NPATH), (NWAVE,NPATH)
        return SPECOUT                                                        # (NWAVE, NPATH)

    # ---- what the three fused gradient routes below share.  Lines of ForwardModel_0.py behind each step:
    #                                                nemesisPTfm    nemesisSOfmg    nemesisLfmg
    #   _fused_setup    copies of the inputs         :1868-1876     :1024-1032      :1413-1421
    #                   consistency checks           (after them)   :1036-1037      :1425-1426
    #                   ILS, wave range, tables      :1890-1895     :1165-1170      :1429-1434
    #   _fused_paths    tangent heights from         :1906-1908     :1180-1182      :1444-1446
    #   _fused_inputs   taucont                      :3989          :3989           :3989
    #   _fused_tail     incpar                       :1925-1928     :1193-1196      :1457-1460
    #   _fused_convg    convolution                  :1986-1994     :1236-1241      :1510-1513
    # nemesisdiscfmg takes _fused_inputs, _fused_tail and _fused_convg(IGEOM=i, :1815-1826) per geometry; its preamble is the
    # reference's own per averaging point (process_IAV :2004-2036).
    def _fused_setup(self, adjust_hydrostat, checks=None):
        """The preamble of a forward-model method with gradients: the X copies of the inputs, the consistency checks (then
        `checks()`, the method's own), the ILS, the calculation range, the tables read over it and the profiles: xmap."""
        from copy import deepcopy
        self.Variables1 = deepcopy(self.Variables)
        self.MeasurementX = deepcopy(self.Measurement)
        self.AtmosphereX = deepcopy(self.Atmosphere)
        self.ScatterX = deepcopy(self.Scatter)
        self.StellarX = deepcopy(self.Stellar)
        self.SurfaceX = deepcopy(self.Surface)
        self.LayerX = deepcopy(self.Layer)
        self.SpectroscopyX = deepcopy(self.Spectroscopy)
        self.CIAX = deepcopy(self.CIA)
        self.check_gas_spec_atm()
        self.check_wave_range_consistency()
        if checks is not None:
            checks()
        self.Measurement.build_ils(IGEOM=0)
        wavecalc_min, wavecalc_max = self.Measurement.calc_wave_range(apply_doppler=True, IGEOM=None)
        if self.SpectroscopyX.NGAS > 0:
            self.SpectroscopyX.read_tables(wavemin=wavecalc_min, wavemax=wavecalc_max)
        self.adjust_hydrostat = adjust_hydrostat
        return self.subprofretg()

    def _fused_paths(self, emtemp=False):
        """NLAYIN (NPATH,), LAYINC, SCALE (LIMAX, NPATH) of PathX, and EMTEMP on request"""
        P = self.PathX
        NPATH = int(P.NPATH)
        out = (np.asarray(P.NLAYIN, dtype=np.int32).reshape(NPATH), np.asarray(P.LAYINC, dtype=np.int32).reshape(-1, NPATH),
               np.asarray(P.SCALE, dtype=np.float64).reshape(-1, NPATH))
        return out + (np.asarray(P.EMTEMP, dtype=np.float64).reshape(-1, NPATH),) if emtemp else out

    def _fused_inputs(self, eng):
        """The table on the engine and what a fused call takes of the layers: the continuum (its parts for the side products),
        the gas amounts, the sizes and igas_map."""
        from types import SimpleNamespace
        S, L, A = self.SpectroscopyX, self.LayerX, self.AtmosphereX
        self._ansfm_upload_table(eng)
        c = SimpleNamespace()
        c.TAUCIA, c.TAUDUST, c.TAURAY, c.dTAUCON = self._ansfm_continuum(True)
        c.taucont = c.TAUCIA + c.TAUDUST + c.TAURAY
        c.f_gas = self._ansfm_layer_inputs()
        c.press, c.temp = np.asarray(L.PRESS, dtype=np.float64), np.asarray(L.TEMP, dtype=np.float64)
        c.NVMR, c.NDUST, c.NPRO, c.NLAY = int(A.NVMR), int(A.NDUST), int(A.NP), int(L.NLAY)
        c.NPAR = c.NVMR + 2 + int(self.ScatterX.NDUST)
        c.igas_map = np.array([A.locate_gas(S.ID[i], S.ISO[i]) for i in range(S.NGAS)], dtype=np.int32)
        return c

    def _fused_tail(self, eng, c, xmap, NGEOM):
        """After the fused call: the side products, then its gradients (NWAVE, NPAR, NLAY, NGEOM) on the device through
        map2pro and map2xvec: dSPECMOD (NWAVE, NGEOM, NX)."""
        S, L = self.SpectroscopyX, self.LayerX
        if self.ansfm_keep_side_products:
            L.TAUGAS = eng.get_taugas(L.NLAY, 0)
            L.TAUTOT = self._ansfm_total_opacity(L.TAUGAS, c.TAUCIA, c.TAUDUST, c.TAURAY)
        incpar = [i for i in range(c.NVMR + 2 + c.NDUST) if np.mean(xmap[:, i, :]) != 0.0]
        eng.map2pro(None, S.NWAVE, c.NVMR, c.NDUST, c.NPRO, NGEOM, np.array([c.NLAY] * NGEOM),
                    np.tile(np.arange(c.NLAY)[:, None], (1, NGEOM)), L.DTE, L.DAM, L.DCO, INCPAR=incpar, to_host=False)
        return eng.map2xvec(None, S.NWAVE, c.NVMR, c.NDUST, c.NPRO, NGEOM, self.Variables.NX, xmap)

    def _fused_convg(self, SPECMOD, dSPECMOD, IGEOM=None):
        """IGEOM None: every geometry at once on MeasurementX.  IGEOM = i: geometry i of Measurement, SPECMOD (NWAVE,) and
        dSPECMOD (NWAVE, NX), with the .fwh file where there is one (:1815-1826)."""
        S = self.SpectroscopyX
        if IGEOM is None:
            M = self.MeasurementX
            if int(S.ILBL) == ILBL_K_TABLES:
                return M.convg(S.WAVE, SPECMOD, dSPECMOD, IGEOM='All')
            return M.lblconvg(S.WAVE, SPECMOD, dSPECMOD, IGEOM='All')
        M = self.Measurement
        if int(self.Spectroscopy.ILBL) == ILBL_K_TABLES:
            FWHMEXIST = self.runname if os.path.exists(self.runname + '.fwh') else ''
            return M.convg(S.WAVE, SPECMOD, dSPECMOD, IGEOM=IGEOM, FWHMEXIST=FWHMEXIST)
        return M.lblconvg(S.WAVE, SPECMOD, dSPECMOD, IGEOM=IGEOM)

    # ---- primary transit with gradients: the depth and its layer gradients collapsed on the device ------------------
    def nemesisPTfm(self, gradients=False):
        """nemesisPTfm (ForwardModel_0.py:1838-1995).  Without gradients: the reference's method, whose CIRSrad is the seam
        above.  With gradients the reference asks CIRSrad for dSPECOUT (NWAVE, NPAR, 2 NLAY, NLAY - 1), maps it to the state
        vector and only then sums the annuli; here `AnsfmEngine.cirsradg_ck_transit` sums the annuli first (the absorbing area
        and its gradient with respect to every layer property), and map2pro / map2xvec run on that (NWAVE, NPAR, NLAY, 1)
        array on the device.  The same steps as the reference's otherwise; its own method takes over for a Telluric object,
        a case CIRSrad would delegate, and more layers than the fused call takes."""
        if gradients is False:
            return super().nemesisPTfm(False)
        if getattr(self, "Telluric", None) is not None:
            return super().nemesisPTfm(gradients)
        eng = get_engine(self.ansfm_device)
        if not hasattr(eng, "cirsradg_ck_transit"):
            return super().nemesisPTfm(gradients)
        from . import transit as _transit

        def one_transit_geometry():
            if int(self.MeasurementX.IFORM) != IFORM_TRANSIT_DEPTH:
                raise ValueError('error in nemesisPTfm :: Measurement unit must be set to TransitDepth (IFORM=2) for primary transit observations')
            if self.MeasurementX.NGEOM != 1:
                raise ValueError('error in nemesisPTfm :: Only one geometry is allowed for primary transit observations (NGEOM=1)')
        xmap = self._fused_setup(True, one_transit_geometry)
        self.LayerX.DUST_UNITS_FLAG = self.AtmosphereX.DUST_UNITS_FLAG
        self.calc_path_PT()
        S, L, P, A = self.SpectroscopyX, self.LayerX, self.PathX, self.AtmosphereX
        imod = np.unique(np.asarray(P.IMOD).astype(int))
        if (not self._ansfm_supported(True) or not self._ansfm_transmission_branch(int(imod[0]))
                or int(S.ILBL) not in (ILBL_K_TABLES, ILBL_LBL_TABLES)):
            return super().nemesisPTfm(gradients)
        NLAYIN, LAYINC, SCALE = self._fused_paths()
        BASEH_TANHE = _transit.tangent_heights_km(L.BASEH, NLAYIN, LAYINC)
        weights = _transit.path_weights(BASEH_TANHE, A.RADIUS)                  # the trapezoid of :1949-1954, by path
        c = self._fused_inputs(eng)
        try:
            AREA, SPECOUT, _ = eng.cirsradg_ck_transit(c.press, c.temp, c.f_gas, c.taucont, c.dTAUCON, c.NVMR, c.NPAR, c.igas_map,
                                                       NLAYIN, LAYINC, SCALE, weights, gradients_on_device=True)
        except NotImplementedError:                 # more layers or paths than the fused call takes
            _note("nemesisPTfm with gradients: more layers or paths than the fused transit call takes; the reference's method runs "
                  "over CIRSrad(return_grad=True) instead")
            return super().nemesisPTfm(gradients)
        _route("nemesisPTfm with gradients: transit depth collapsed over the paths on the device")
        dAREA = self._fused_tail(eng, c, xmap, 1)                               # (NWAVE, 1, NX)
        area_star = np.pi * ((self.StellarX.RADIUS * 1.0e3) ** 2)               # :1941-1944
        area_planet_disk = np.pi * ((A.RADIUS + BASEH_TANHE[0] * 1.0e3) ** 2)
        SPECMOD = np.zeros((S.NWAVE, self.MeasurementX.NGEOM))
        dSPECMOD = np.zeros((S.NWAVE, self.MeasurementX.NGEOM, self.Variables.NX))
        SPECMOD[:, 0] = AREA
        dSPECMOD[:, 0, :] = dAREA[:, 0, :]
        SPECMOD = (SPECMOD + area_planet_disk) / area_star * 100.               # :1963-1966
        dSPECMOD = dSPECMOD / area_star * 100.
        SPECONV, dSPECONV = self._fused_convg(SPECMOD, dSPECMOD)
        SPECONV, dSPECONV = self.subspecret(SPECONV, dSPECONV)
        return SPECONV, dSPECONV

    # ---- solar occultation with gradients: the tangent paths mixed to the geometries on the device ------------------
    def nemesisSOfmg(self):
        """nemesisSOfmg (ForwardModel_0.py:983-1249), plain branch (:1160-1247).  The reference asks CIRSrad for dSPECOUT
        (NWAVE, NPAR, LIMAX, NPATH), maps it to the state vector path by path and only then interpolates the paths to the
        tangent heights of the measurement (:1208-1232); every step after the transmission is linear, so here ONE
        `AnsfmEngine.cirsradg_ck_occultation` call applies the interpolation first (`occultation.tangent_mix`) and map2pro /
        map2xvec run on that (NWAVE, NPAR, NLAY, NGEOM) array on the device.  The same steps as the reference's otherwise.  Its
        own method, whose CIRSrad(return_grad=True) is the seam above, takes over for the AOTF branch, a Telluric object,
        runtime line-by-line, a case CIRSrad would delegate, an engine without the call and one that refuses it."""
        if getattr(self.Measurement, "NORDERS_AOTF", None) is not None or getattr(self, "Telluric", None) is not None:
            return super().nemesisSOfmg()
        eng = get_engine(self.ansfm_device)
        if not hasattr(eng, "cirsradg_ck_occultation"):
            return super().nemesisSOfmg()
        from . import occultation as _occ
        xmap = self._fused_setup(False)
        self.calc_pathg_SO()
        S, L, P, M = self.SpectroscopyX, self.LayerX, self.PathX, self.MeasurementX
        imod = np.unique(np.asarray(P.IMOD).astype(int))
        if (not self._ansfm_supported(True) or not self._ansfm_transmission_branch(int(imod[0]))
                or int(S.ILBL) not in (ILBL_K_TABLES, ILBL_LBL_TABLES)):
            return super().nemesisSOfmg()
        NLAYIN, LAYINC, SCALE = self._fused_paths()
        mix = _occ.tangent_mix(_occ.tangent_heights_km(L.BASEH, NLAYIN, LAYINC), M.TANHE)      # :1211-1232
        c = self._fused_inputs(eng)
        xf = None
        if int(M.IFORM) == IFORM_ATMOSPHERIC_TRANSMISSION:                      # :4119-4127: times the solar flux
            import scipy.interpolate
            self.StellarX.calc_solar_flux()
            xf = scipy.interpolate.interp1d(self.StellarX.WAVE, self.StellarX.SOLFLUX)(S.WAVE)
        try:
            MOD, SPECOUT, _ = eng.cirsradg_ck_occultation(c.press, c.temp, c.f_gas, c.taucont, c.dTAUCON, c.NVMR, c.NPAR, c.igas_map,
                                                          NLAYIN, LAYINC, SCALE, mix=mix, xfac=xf, gradients_on_device=True)
        except NotImplementedError:                 # more layers or paths than the fused call takes, or no room for dMOD
            _note("nemesisSOfmg: the fused occultation call refused the case (layers, paths or the size of dMOD); the reference's "
                  "method runs over CIRSrad(return_grad=True) instead")
            return super().nemesisSOfmg()
        _route("nemesisSOfmg: tangent paths mixed to the geometries on the device")
        dSPECMOD = self._fused_tail(eng, c, xmap, int(M.NGEOM))                 # (NWAVE, NGEOM, NX)
        SPECMOD = np.array(MOD)
        SPECONV, dSPECONV = self._fused_convg(SPECMOD, dSPECMOD)
        dSPECONV = self.subspeconv(S.WAVE, SPECMOD, dSPECONV)                   # :1244
        SPECONV, dSPECONV = self.subspecret(SPECONV, dSPECONV)                  # :1247
        return SPECONV, dSPECONV

    # ---- limb thermal emission with gradients: the tangent paths mixed to the geometries on the device ---------------
    def nemesisLfmg(self):
        """nemesisLfmg (ForwardModel_0.py:1372-1521).  The reference asks CIRSrad for dSPECOUT (NWAVE, NPAR, LIMAX, NPATH) of
        the thermal-emission branch, maps it to the state vector path by path and only then interpolates the paths to the
        tangent heights of the measurement (:1475-1496); every step after the radiative transfer is linear, so here ONE
        `AnsfmEngine.cirsradg_ck_limb` call applies the interpolation first (`limb.tangent_mix`) and map2pro / map2xvec run on
        that (NWAVE, NPAR, NLAY, NGEOM) array on the device.  The same steps as the reference's otherwise.  Its own method,
        whose CIRSrad(return_grad=True) is the seam above, takes over for a Telluric object, runtime line-by-line, a case
        CIRSrad would delegate, a path calculation that is not thermal emission, a path that ends at the lower boundary, an
        engine without the call and one that refuses it."""
        if getattr(self, "Telluric", None) is not None:
            return super().nemesisLfmg()
        eng = get_engine(self.ansfm_device)
        if not hasattr(eng, "cirsradg_ck_limb"):
            return super().nemesisLfmg()
        from . import limb as _limb
        xmap = self._fused_setup(False)
        self.calc_pathg_L()
        S, L, P, M = self.SpectroscopyX, self.LayerX, self.PathX, self.MeasurementX
        imod = np.unique(np.asarray(P.IMOD).astype(int))
        if (not self._ansfm_supported(True) or int(S.ILBL) not in (ILBL_K_TABLES, ILBL_LBL_TABLES)
                or self._ansfm_transmission_branch(int(imod[0])) or (int(imod[0]) & IMOD_ABSORBTION)
                or not (int(imod[0]) & IMOD_THERMAL_EMISSION)):                 # dispatch order :4478-4489
            return super().nemesisLfmg()
        NLAYIN, LAYINC, SCALE, EMTEMP = self._fused_paths(emtemp=True)
        mix = _limb.tangent_mix(_limb.tangent_heights_km(L.BASEH, NLAYIN, LAYINC), M.TANHE)    # :1475-1496
        c = self._fused_inputs(eng)
        xf, _ = self._ansfm_units_and_surface()                                 # :4158-4168
        try:
            MOD, SPECOUT, _ = eng.cirsradg_ck_limb(int(M.ISPACE), c.press, c.temp, c.f_gas, c.taucont, c.dTAUCON, c.NVMR, c.NPAR,
                                                   c.igas_map, NLAYIN, LAYINC, SCALE, EMTEMP, mix=mix, xfac=xf,
                                                   gradients_on_device=True)
        except NotImplementedError:                 # more layers than the fused call takes, a path that ends at the lower boundary
            #                                         (:6479-6483: the engine makes that test), or no room for dMOD or the scratch
            _note("nemesisLfmg: the fused limb call refused the case (layers, a path to the lower boundary, the size of dMOD or of "
                  "the scratch); the reference's method runs over CIRSrad(return_grad=True) instead")
            return super().nemesisLfmg()
        _route("nemesisLfmg: tangent paths mixed to the geometries on the device")
        dSPECMOD = self._fused_tail(eng, c, xmap, int(M.NGEOM))                 # (NWAVE, NGEOM, NX)
        SPECMOD = np.array(MOD)
        if int(M.IFORM) == IFORM_INTEGRATED_RADIANCE:                           # :1500-1504
            SPECONV, dSPECONV = M.integrate_filterg(S.WAVE, SPECMOD, dSPECMOD, IGEOM='All')
        else:
            SPECONV, dSPECONV = self._fused_convg(SPECMOD, dSPECMOD)
            dSPECONV = self.subspeconv(S.WAVE, SPECMOD, dSPECONV)               # :1516
        SPECONV, dSPECONV = self.subspecret(SPECONV, dSPECONV)                  # :1519
        return SPECONV, dSPECONV

    # ---- disc average with gradients: the averaging points mixed on the device ----------------------------------------
    def _ansfm_disc_point(self, IGEOM, IAV):
        """process_IAV(return_grad=True) up to calc_pathg (:2004-2036): xmap"""
        from copy import deepcopy
        self.select_Measurement(IGEOM, IAV)
        self.AtmosphereX = deepcopy(self.Atmosphere)
        self.ScatterX = deepcopy(self.Scatter)
        self.StellarX = deepcopy(self.Stellar)
        self.SurfaceX = deepcopy(self.Surface)
        self.LayerX = deepcopy(self.Layer)
        self.CIAX = deepcopy(self.CIA)
        self.TelluricX = deepcopy(self.Telluric)
        MX = self.MeasurementX
        if MX.EMISS_ANG[0, 0] >= 0.0:
            self.ScatterX.SOL_ANG = MX.SOL_ANG[0, 0]
            self.ScatterX.EMISS_ANG = MX.EMISS_ANG[0, 0]
            self.ScatterX.AZI_ANG = MX.AZI_ANG[0, 0]
        else:
            self.ScatterX.SOL_ANG = MX.TANHE[0, 0]
            self.ScatterX.EMISS_ANG = MX.EMISS_ANG[0, 0]
        xmap = self.subprofretg()
        self.LayerX.DUST_UNITS_FLAG = self.AtmosphereX.DUST_UNITS_FLAG
        self.calc_pathg()
        return xmap

    def _ansfm_disc_fused(self, eng, IGEOM, NAV):
        """One geometry through ONE `cirsradg_ck_disc` call: SPEC (NWAVE,), dSPEC (NWAVE, NX), or None where the fused call does
        not take the geometry (the caller then runs the points through process_IAV)."""
        from . import disc as _disc
        M = self.Measurement
        if np.any(np.asarray(M.EMISS_ANG)[IGEOM, :NAV] < 0.0):                  # limb points: other layers per point
            return None
        points = []
        for IAV in range(NAV):
            xmap = self._ansfm_disc_point(IGEOM, IAV)
            points.append((self.LayerX, self.PathX, self.SurfaceX, xmap))
            if IAV == 0:                            # what declines the geometry shows at its first point: the others are spared
                S = self.SpectroscopyX
                imod = np.unique(np.asarray(self.PathX.IMOD).astype(int))
                if (not self._ansfm_supported(True) or int(S.ILBL) not in (ILBL_K_TABLES, ILBL_LBL_TABLES)
                        or self._ansfm_transmission_branch(int(imod[0])) or (int(imod[0]) & IMOD_ABSORBTION)
                        or not (int(imod[0]) & IMOD_THERMAL_EMISSION)):         # dispatch order :4478-4489
                    return None
        seq = _disc.shared_sequence(points)
        imod0 = np.asarray(points[0][1].IMOD)       # the first point's was tested above; the others must name the same calculation
        if seq is None or any(not np.array_equal(np.asarray(P.IMOD), imod0) for _, P, _, _ in points[1:]):
            return None
        LAYINC, EMTEMP, SCALE = seq
        c = self._fused_inputs(eng)
        xf, emissivity = self._ansfm_units_and_surface()                        # :4158-4189
        try:
            MOD, _, dTSMOD, _ = eng.cirsradg_ck_disc(int(self.MeasurementX.ISPACE), c.press, c.temp, c.f_gas, c.taucont, c.dTAUCON,
                                                     c.NVMR, c.NPAR, c.igas_map, LAYINC, SCALE, EMTEMP, float(self.SurfaceX.TSURF),
                                                     EMISSIVITY=emissivity, mix=_disc.average_mix(np.asarray(M.WGEOM)[IGEOM, :NAV]),
                                                     xfac=xf, gradients_on_device=True)
        except NotImplementedError:                 # more layers than the fused call takes, or no room for dMOD or the scratch
            _note("nemesisdiscfmg: the fused disc call refused the case (layers, the size of dMOD or of the scratch); the averaging "
                  "points run one by one over CIRSrad(return_grad=True) instead")
            return None
        _route("nemesisdiscfmg: averaging points mixed on the device")
        dSPEC = np.array(self._fused_tail(eng, c, xmap, 1)[:, 0, :])             # (NWAVE, NX)
        if self.Variables.JSURF >= 0:                                           # :2062-2063 carried through the sum
            dSPEC[:, self.Variables.JSURF] = dTSMOD[:, 0]
        return np.array(MOD[:, 0]), dSPEC

    def nemesisdiscfmg(self):
        """nemesisdiscfmg (ForwardModel_0.py:1719-1834).  For every averaging point of a geometry the reference runs
        process_IAV(return_grad=True) -- paths, CIRSrad with dSPECOUT (NWAVE, NPAR, NLAYIN, 1), map2pro, map2xvec -- and only then
        forms the weighted sum with WGEOM (:1789-1794).  Every step after the radiative transfer is linear and the points of a
        geometry are paths through one layer sequence that differ in SCALE only, so here ONE `AnsfmEngine.cirsradg_ck_disc` call
        per geometry forms the sum first (`disc.average_mix`); the gas stage and the gradient merge run once, and map2pro /
        map2xvec run on that (NWAVE, NPAR, NLAY, 1) array on the device.  The same steps as the reference's otherwise.  A geometry
        the fused call does not take -- a point with EMISS_ANG < 0, points whose layers or paths differ in any bit
        (`disc.shared_sequence`), runtime line-by-line, a case CIRSrad would delegate, a path calculation that is not thermal
        emission, an engine that refuses -- runs its points through process_IAV in this process, whose CIRSrad(return_grad=True)
        is the seam above, and weights them as the reference does.  NCores is not used: no joblib workers on one GPU.  The
        reference's method takes over for a Telluric object and an engine without the call."""
        from copy import deepcopy
        if getattr(self, "Telluric", None) is not None:
            return super().nemesisdiscfmg()
        eng = get_engine(self.ansfm_device)
        if not hasattr(eng, "cirsradg_ck_disc"):
            return super().nemesisdiscfmg()
        if self.Atmosphere.NLOCATIONS > 1:                                      # :1750-1758
            raise ValueError('error in nemesisdiscfmg :: archNEMESIS has not been setup for dealing with multiple locations yet')
        if self.Surface.NLOCATIONS > 1:
            raise ValueError('error in nemesisdiscfmg :: archNEMESIS has not been setup for dealing with multiple locations yet')
        self.check_gas_spec_atm()
        self.check_wave_range_consistency()
        if getattr(self, "NCores", None) is not None and int(self.NCores) > 1:
            _note("nemesisdiscfmg(NCores > 1): the averaging points are mixed in one call on the GPU (or run one after the other in "
                  "this process), not in joblib workers")
        M = self.Measurement
        SPECONV = np.zeros(M.MEAS.shape)
        dSPECONV = np.zeros((M.NCONV.max(), M.NGEOM, self.Variables.NX))
        for IGEOM in range(M.NGEOM):
            M.build_ils(IGEOM=IGEOM)                                            # :1767-1773
            wavecalc_min, wavecalc_max = M.calc_wave_range(apply_doppler=True, IGEOM=IGEOM)
            self.SpectroscopyX = deepcopy(self.Spectroscopy)
            if self.SpectroscopyX.NGAS > 0:
                self.SpectroscopyX.read_tables(wavemin=wavecalc_min, wavemax=wavecalc_max)
            NAV = int(M.NAV[IGEOM])
            fused = self._ansfm_disc_fused(eng, IGEOM, NAV)
            if fused is not None:
                SPEC, dSPEC = fused
            else:                                                               # :1776-1794, in this process
                SPEC, dSPEC = 0.0, 0.0
                for IAV in range(NAV):
                    s1, d1 = self.process_IAV(IAV, IGEOM, return_grad=True)
                    SPEC = SPEC + s1 * M.WGEOM[IGEOM, IAV]
                    dSPEC = dSPEC + d1 * M.WGEOM[IGEOM, IAV]
            SPECONV1, dSPECONV1 = self._fused_convg(SPEC, dSPEC, IGEOM=IGEOM)  # :1815-1826
            n = M.NCONV[IGEOM]
            SPECONV[0:n, IGEOM] = SPECONV1[0:n]
            dSPECONV[0:n, IGEOM, :] = dSPECONV1[0:n, :]
        SPECONV, dSPECONV = self.subspecret(SPECONV, dSPECONV)                  # :1832
        return SPECONV, dSPECONV


def make_gpu_forward_model(reference_forward_model_cls, device=0):
    """Subclass of the reference's ForwardModel_0 with the GPU CIRSrad seam and `jacobian_nemesis` without the joblib
    fan-out (jacobian_dropin.JacobianGPU)."""
    from .jacobian_dropin import JacobianGPU
    return type("ForwardModel_0", (JacobianGPU, CIRSradGPU, reference_forward_model_cls),
                {"ansfm_device": device, "__doc__": reference_forward_model_cls.__doc__})


def install_gpu_forward_model(device=0):
    """Make the retrieval drivers build the GPU forward model: `coreretOE` imports the class at call time (`from archnemesis
    import ForwardModel_0`, OptimalEstimation_0.py:1255) and `Retrievals` / `NestedSampling_0` build `ans.ForwardModel_0(...)`
    (Retrievals.py:102, :181, :256), so the package attribute `archnemesis.ForwardModel_0` is what has to name the subclass
    (the submodule of the same name stays reachable through importlib / sys.modules).  The reference's class is kept as
    `archnemesis._ansfm_reference_ForwardModel_0`; calling this twice is harmless.  Returns the subclass."""
    import importlib
    pkg = importlib.import_module("archnemesis")
    ref = getattr(pkg, "_ansfm_reference_ForwardModel_0", None)
    if ref is None:
        ref = pkg.ForwardModel_0
        if not isinstance(ref, type):          # the attribute named the submodule (no star import of the class): take the class
            ref = importlib.import_module("archnemesis.ForwardModel_0").ForwardModel_0
        pkg._ansfm_reference_ForwardModel_0 = ref
    cls = make_gpu_forward_model(ref, device)
    pkg.ForwardModel_0 = cls
    for modname in ("archnemesis.OptimalEstimation_0", "archnemesis.Retrievals", "archnemesis.NestedSampling_0"):
        mod = sys.modules.get(modname)
        if mod is not None and isinstance(getattr(mod, "ForwardModel_0", None), type):
            mod.ForwardModel_0 = cls               # module-level `from archnemesis import ForwardModel_0` bindings
    return cls


def uninstall_gpu_forward_model():
    import importlib
    pkg = importlib.import_module("archnemesis")
    ref = getattr(pkg, "_ansfm_reference_ForwardModel_0", None)
    if ref is not None:
        pkg.ForwardModel_0 = ref
        for modname in ("archnemesis.OptimalEstimation_0", "archnemesis.Retrievals", "archnemesis.NestedSampling_0"):
            mod = sys.modules.get(modname)
            if mod is not None and isinstance(getattr(mod, "ForwardModel_0", None), type):
                mod.ForwardModel_0 = ref


def install_gpu_scattering_core(device=0):
    """Route the reference's multiple-scattering core through the GPU.

    ForwardModel_0.scloud11wave (ForwardModel_0.py:5018) prepares RADGROUND/BB/FRAC/OMEGA/PHASE_ARRAY on the host
    and imports `scloud11wave_core` from archnemesis.Multiple_Scattering_Core at call time (:5050); replacing that
    module attribute keeps all of the reference's host preparation and swaps only the core (K7).  More than 16 paths are run
    in groups of 16 by the engine; more than 32 streams go to the reference's own function."""
    import importlib
    msc = importlib.import_module("archnemesis.Multiple_Scattering_Core")
    eng = get_engine(device)
    ref_core = getattr(msc, "_ansfm_reference_core", None) or msc.scloud11wave_core

    def scloud11wave_core(phasarr, radg, sol_angs, emiss_angs, solar, aphis, lowbc, brdf_matrix, mu1, wt1, nf, vwaves, bnu,
                          taus, tauray, omegas_s, nphi, iray, imie, lfrac):
        try:
            return eng.scloud11wave_core(phasarr, radg, sol_angs, emiss_angs, solar, aphis, int(lowbc), brdf_matrix, mu1, wt1,
                                         nf, vwaves, bnu, taus, tauray, omegas_s, nphi, int(iray), int(imie), lfrac)
        except NotImplementedError:
            _delegate("scloud11wave_core with more than 32 streams")
            return ref_core(phasarr, radg, sol_angs, emiss_angs, solar, aphis, lowbc, brdf_matrix, mu1, wt1, nf, vwaves, bnu,
                            taus, tauray, omegas_s, nphi, iray, imie, lfrac)

    msc._ansfm_reference_core = ref_core
    msc.scloud11wave_core = scloud11wave_core
    return scloud11wave_core


def install_gpu_line_kernel(device=0):
    """Route LineData_0.add_line_set_monochromatic_absorption (LineData_0.py:280) through the GPU for the line shapes
    that are built (voigt / lorentz / gaussian); other `lineshape_fn` objects go to the reference's own kernel."""
    import importlib
    ld = importlib.import_module("archnemesis.LineData_0")
    ls = importlib.import_module("archnemesis.lineshape")
    eng = get_engine(device)
    ref_fn = getattr(ld, "_ansfm_reference_line_kernel", None) or ld.add_line_set_monochromatic_absorption
    ids = {id(ls.voigt): 0, id(ls.lorentz): 4, id(ls.gaussian): 12}

    def add_line_set_monochromatic_absorption(wn_grid, lineshape_fn, t_calc, t_ref, p_calc, p_ref, q_ratio,
                                              isotopic_abundance, isotopic_mass, mol_mix_frac, broadening_params, nu, sw,
                                              e_lower, stimulated_emission_at_t_ref, out, store=None, s_floor=0,
                                              wn_calc_window=25.0, wn_approx_window=75.0):
        lid = ids.get(id(lineshape_fn))
        ok = (lid is not None and isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous
              and (store is None or (store.dtype == np.float64 and store.flags.c_contiguous)))
        if not ok:
            _delegate("line shape / buffer layout of add_line_set_monochromatic_absorption")
            return ref_fn(wn_grid, lineshape_fn, t_calc, t_ref, p_calc, p_ref, q_ratio, isotopic_abundance, isotopic_mass,
                          mol_mix_frac, broadening_params, nu, sw, e_lower, stimulated_emission_at_t_ref, out, store, s_floor,
                          wn_calc_window, wn_approx_window)
        eng.add_line_set_monochromatic_absorption(wn_grid, lid, t_calc, t_ref, p_calc, p_ref, q_ratio, isotopic_abundance,
                                                  isotopic_mass, mol_mix_frac, broadening_params, nu, sw, e_lower,
                                                  stimulated_emission_at_t_ref, out, store, s_floor, wn_calc_window,
                                                  wn_approx_window)
        return

    ld._ansfm_reference_line_kernel = ref_fn
    ld.add_line_set_monochromatic_absorption = add_line_set_monochromatic_absorption
    return add_line_set_monochromatic_absorption


PC_MAX_NEIGHBOUR_BINS = 8              # kPcMaxNeighbours of the pseudo-continuum kernels


def install_gpu_pseudo_continuum(device=0):
    """Route LineData_0.add_pseudo_continuum_monochromatic_absorption (LineData_0.py:486; the class method resolves the
    module attribute at call time, :1378) -- the pseudo-continuum of the weak lines, the second term of every default
    runtime line-by-line opacity -- through the GPU.  To the reference's own function go: line shapes that are not built,
    an `out` / `store` / `store_x` that is not a contiguous float64 array, bins whose lower edges are not ascending (or whose
    widths are not positive), more than 8 neighbour bins, and `store_x is None` with fewer grid points than bins (where
    the reference raises IndexError).  The reference's scratch arrays store_y / store_z are left as they are."""
    import importlib
    ld = importlib.import_module("archnemesis.LineData_0")
    ls = importlib.import_module("archnemesis.lineshape")
    eng = get_engine(device)
    ref_fn = getattr(ld, "_ansfm_reference_pseudo_continuum", None) or ld.add_pseudo_continuum_monochromatic_absorption
    ids = {id(ls.voigt): 0, id(ls.lorentz): 4, id(ls.gaussian): 12}

    def _f8c(a, size):
        return isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.size == size

    def add_pseudo_continuum_monochromatic_absorption(wn_grid, lineshape_fn, t_calc, t_ref, p_calc, p_ref, q_ratio,
                                                      isotopic_abundance, isotopic_mass, mol_mix_frac,
                                                      lsw_mean_broadening_params, wn_bin_centers, wn_bin_widths, sw_sum,
                                                      lsw_mean_e_lower, out, store=None, store_x=None, store_y=None,
                                                      store_z=None, n_neighbour_bins=3):
        lid = ids.get(id(lineshape_fn))
        c, w = np.asarray(wn_bin_centers, dtype=np.float64), np.asarray(wn_bin_widths, dtype=np.float64)
        N, nw = c.shape[0], np.shape(wn_grid)[0]
        why = None
        if lid is None:
            why = "line shape of add_pseudo_continuum_monochromatic_absorption"
        elif not (_f8c(out, nw) and out.ndim == 1 and (store is None or _f8c(store, 3 * N))
                  and (store_x is None or _f8c(store_x, N))):
            why = "buffer layout of add_pseudo_continuum_monochromatic_absorption"
        elif not (np.all(w > 0.0) and np.all(np.diff(c - w / 2.0) >= 0.0)):
            why = "pseudo-continuum bins whose lower edges are not ascending"
        elif int(n_neighbour_bins) > PC_MAX_NEIGHBOUR_BINS or int(n_neighbour_bins) < 0:
            why = "pseudo-continuum with more than %d neighbour bins" % PC_MAX_NEIGHBOUR_BINS
        elif store_x is None and nw < N:
            why = "pseudo-continuum without store_x on a grid shorter than the bins"
        if why is not None:
            _delegate(why)
            return ref_fn(wn_grid, lineshape_fn, t_calc, t_ref, p_calc, p_ref, q_ratio, isotopic_abundance, isotopic_mass,
                          mol_mix_frac, lsw_mean_broadening_params, wn_bin_centers, wn_bin_widths, sw_sum, lsw_mean_e_lower,
                          out, store, store_x, store_y, store_z, n_neighbour_bins)
        eng.add_pseudo_continuum_monochromatic_absorption(wn_grid, lid, t_calc, t_ref, p_calc, p_ref, q_ratio,
                                                          isotopic_abundance, isotopic_mass, mol_mix_frac,
                                                          lsw_mean_broadening_params, c, w, sw_sum, lsw_mean_e_lower, out,
                                                          store, store_x, int(n_neighbour_bins))
        return

    ld._ansfm_reference_pseudo_continuum = ref_fn
    ld.add_pseudo_continuum_monochromatic_absorption = add_pseudo_continuum_monochromatic_absorption
    return add_pseudo_continuum_monochromatic_absorption


MIE_MEMO_ENTRIES = 8                   # size distributions the Mie hook remembers (a Jacobian perturbs one parameter at a time)


def install_gpu_mie(device=0):
    """Route the module-level Scatter_0.makephase (Scatter_0.py:1828; the class method resolves the module attribute at call
    time, :1340) -- Mie theory integrated over a particle size distribution, which model 444 recomputes in every forward
    model -- through the GPU for iscat 1 .. 4.  iscat 5 / 6 / 7 (isotropic, Henyey-Greenstein, dipole) are closed forms and
    are forwarded to the reference's function; that is no delegation.  A call the engine refuses (a Mie series the reference
    gives up on, an open range that does not end, an angle outside [0, 90]) is delegated, so that the reference fails its
    own way.  The hook remembers the last MIE_MEMO_ENTRIES results under the bytes of every argument: the NX + 1 states of a
    staged Jacobian repeat all but a few size distributions bit for bit.  A remembered call returns copies, because the class
    method scales and permutes `phas` in place (:1343-1344).  summary()["routes"] counts `mie` and `mie (memo)`."""
    import importlib
    from collections import OrderedDict
    from ._lib import AnsfmError
    sc = importlib.import_module("archnemesis.Scatter_0")
    eng = get_engine(device)
    ref_fn = getattr(sc, "_ansfm_reference_makephase", None) or sc.makephase
    memo = OrderedDict()

    def makephase(wavel, iscat, dsize, rs, refindx, theta):
        if int(iscat) not in (1, 2, 3, 4):
            return ref_fn(wavel, iscat, dsize, rs, refindx, theta)
        args = [np.ascontiguousarray(a, dtype=np.float64) for a in (wavel, dsize, rs, refindx, theta)]
        key = (int(iscat),) + tuple((a.shape, a.tobytes()) for a in args)
        hit = memo.get(key)
        if hit is not None:
            memo.move_to_end(key)
            _route("mie (memo)")
            return tuple(a.copy() for a in hit)
        try:
            out = eng.mie_makephase(args[0], int(iscat), args[1], args[2], args[3], args[4])
        except (ValueError, NotImplementedError, AnsfmError):
            _delegate("makephase: a Mie integration the engine gives up on")
            return ref_fn(wavel, iscat, dsize, rs, refindx, theta)
        _route("mie")
        memo[key] = tuple(np.array(a, dtype=np.float64) for a in out[:4])
        while len(memo) > MIE_MEMO_ENTRIES:
            memo.popitem(last=False)
        return tuple(a.copy() for a in memo[key])

    sc._ansfm_reference_makephase = ref_fn
    sc.makephase = makephase
    return makephase


HG_FIT_MEMO_ENTRIES = 8                # fits the Henyey-Greenstein hook remembers: one per size distribution of the Mie memo
HG_FIT_NPHASE_CAP = AnsfmEngine.HG_FIT_NPHASE_CAP      # angles of a phase function the engine's hg_fit takes


def install_gpu_hg_fit(device=0):
    """Route the module-level Scatter_0.subfithgm (Scatter_0.py:1948; the class method Scatter_0.makephase resolves the
    module attribute at call time, :1366) -- the Levenberg-Marquardt fit of (f, g1, g2) to every wavelength's phase function
    that follows the Mie integration when IMIE = 0 -- through the GPU.  A call the engine refuses (arguments that are not a
    1-D and a 2-D float64 array of matching shapes, more than HG_FIT_NPHASE_CAP angles, an engine error such as a singular
    fit) is delegated, so that the reference fails its own way.  The hook remembers the last HG_FIT_MEMO_ENTRIES results under
    the bytes of (theta, phase), as the Mie hook does with its arguments, and a remembered call returns copies.
    summary()["routes"] counts `hg fit` and `hg fit (memo)`."""
    import importlib
    from collections import OrderedDict
    from ._lib import AnsfmError
    sc = importlib.import_module("archnemesis.Scatter_0")
    eng = get_engine(device)
    ref_fn = getattr(sc, "_ansfm_reference_subfithgm", None) or sc.subfithgm
    memo = OrderedDict()

    def subfithgm(theta, phase):
        f8 = lambda a, ndim: isinstance(a, np.ndarray) and a.dtype == np.float64 and a.ndim == ndim
        if not (f8(theta, 1) and f8(phase, 2) and phase.shape[1] == theta.shape[0] and phase.shape[0] >= 1 and theta.shape[0] >= 1):
            _delegate("subfithgm: arguments that are not float64 arrays (nphase,) and (nwave, nphase)")
            return ref_fn(theta, phase)
        if theta.shape[0] > HG_FIT_NPHASE_CAP:
            _delegate("subfithgm: more than %d angles" % HG_FIT_NPHASE_CAP)
            return ref_fn(theta, phase)
        args = (np.ascontiguousarray(theta), np.ascontiguousarray(phase))
        key = tuple((a.shape, a.tobytes()) for a in args)
        hit = memo.get(key)
        if hit is not None:
            memo.move_to_end(key)
            _route("hg fit (memo)")
            return tuple(a.copy() for a in hit)
        try:
            out = eng.hg_fit(args[0], args[1])
        except (ValueError, NotImplementedError, AnsfmError):
            _delegate("subfithgm: a fit the engine gives up on")
            return ref_fn(theta, phase)
        _route("hg fit")
        memo[key] = tuple(np.array(a, dtype=np.float64) for a in out[:4])
        while len(memo) > HG_FIT_MEMO_ENTRIES:
            memo.popitem(last=False)
        return tuple(a.copy() for a in memo[key])

    sc._ansfm_reference_subfithgm = ref_fn
    sc.subfithgm = subfithgm
    return subfithgm


def install_gpu_phase(device=0):
    """Route Scatter_0.calc_phase (Scatter_0.py:760, all three IMIE modes) and calc_phase_ray (:834) through the GPU
    (AnsfmEngine.calc_phase / calc_phase_ray).  Where the reference raises a ValueError -- its range test, an angle outside
    Scatter.THETA with IMIE 1 -- the reference's own method is called and raises it, message included.  Delegated (DELEGATED,
    an error under set_strict(True)): a Scatter.WAVE that is not strictly ascending (interp1d would sort it), arrays that
    are not float64, and what the engine does not take (more than 7 populations through a resident source).
    summary()["routes"] counts `phase`.  Not part of install_all: Henyey-Greenstein and Legendre values move by ulps against
    NumPy's cos and pow, and drop-in tests compare some routes bit for bit (INTEGRATION.md says how to switch it on)."""
    import importlib
    from ._lib import AnsfmError
    sc = importlib.import_module("archnemesis.Scatter_0")
    cls = sc.Scatter_0
    eng = get_engine(device)
    ref_phase = getattr(cls, "_ansfm_reference_calc_phase", None) or cls.calc_phase
    ref_ray = getattr(cls, "_ansfm_reference_calc_phase_ray", None) or cls.calc_phase_ray
    f8 = lambda a, ndim: isinstance(a, np.ndarray) and a.dtype == np.float64 and a.ndim == ndim

    def calc_phase(self, Theta, Wave):
        imie = int(self.IMIE)
        names = {0: ("F", "G1", "G2"), 1: ("PHASE",), 2: ("WLPOL",)}.get(imie)
        if names is None:
            return ref_phase(self, Theta, Wave)             # 'IMIE value not valid'
        tabs = [getattr(self, n, None) for n in names]
        SW = getattr(self, "WAVE", None)
        if not (f8(Theta, 1) and f8(Wave, 1) and f8(SW, 1) and all(f8(t, 2 if imie == 0 else 3) for t in tabs) and
                (imie != 1 or f8(getattr(self, "THETA", None), 1)) and Theta.size and Wave.size and SW.size >= 2):
            _delegate("calc_phase: arguments or tables that are not float64 arrays")
            return ref_phase(self, Theta, Wave)
        if not np.all(np.diff(SW) > 0) or (imie == 1 and not np.all(np.diff(self.THETA) > 0)):
            _delegate("calc_phase: a Scatter.WAVE or Scatter.THETA that is not strictly ascending")
            return ref_phase(self, Theta, Wave)
        if SW.min() > (1. + 1.0e-6) * Wave.min() or SW.max() < (1. - 1.0e-6) * Wave.max():
            return ref_phase(self, Theta, Wave)             # the reference's ValueError
        if imie == 1 and (Theta.min() < self.THETA[0] or Theta.max() > self.THETA[-1] or np.isnan(Theta).any()):
            return ref_phase(self, Theta, Wave)             # interp1d's ValueError
        tab = np.array(tabs) if imie == 0 else (tabs[0] if imie == 1 else tabs[0][:, :int(self.NLPOL)])
        try:
            out = eng.calc_phase(imie, SW, self.THETA if imie == 1 else None, tab, Theta, Wave)
        except (ValueError, NotImplementedError, AnsfmError):
            _delegate("calc_phase: a call the engine does not take")
            return ref_phase(self, Theta, Wave)
        _route("phase")
        return out

    def calc_phase_ray(self, Theta):
        if not (f8(Theta, 1) and Theta.size):
            _delegate("calc_phase_ray: an argument that is not a float64 array")
            return ref_ray(self, Theta)
        out = eng.calc_phase_ray(Theta)
        _route("phase")
        return out

    cls._ansfm_reference_calc_phase, cls._ansfm_reference_calc_phase_ray = ref_phase, ref_ray
    cls.calc_phase, cls.calc_phase_ray = calc_phase, calc_phase_ray
    return calc_phase, calc_phase_ray


def aerosol_memo_capacity(variables):
    """Entries the Mie and the fit memo need so that a staged Jacobian computes every distinct aerosol state once:
    max(8, 1 + the state-vector elements of the models whose class calls Scatter.makephase).  A staged route walks
    `for geometry: for state: for averaging point`, so a memo smaller than the distinct aerosol states has dropped the first
    state when the next geometry asks for it again, and every geometry recomputes them all.  Model 444 carries two
    size-distribution elements beside its imaginary-index array: more than five of those are more than eight states."""
    import inspect
    n = 0
    for model in getattr(variables, "models", None) or ():
        try:
            calls = "makephase" in inspect.getsource(type(model))
        except (OSError, TypeError):
            calls = False
        if calls:
            n += int(getattr(model, "n_state_vector_entries", 0))
    return max(MIE_MEMO_ENTRIES, HG_FIT_MEMO_ENTRIES, 1 + n)


class raised_memo_capacity:
    """with raised_memo_capacity(variables): the Mie and fit memos hold aerosol_memo_capacity(variables) entries inside the
    block and their defaults again after it (a memo that has grown is cut back by its next new entry).  No result changes:
    a memo only spares the engine a call."""

    def __init__(self, variables):
        self.variables = variables

    def __enter__(self):
        global MIE_MEMO_ENTRIES, HG_FIT_MEMO_ENTRIES
        self.saved = (MIE_MEMO_ENTRIES, HG_FIT_MEMO_ENTRIES)
        MIE_MEMO_ENTRIES = HG_FIT_MEMO_ENTRIES = aerosol_memo_capacity(self.variables)
        return self

    def __exit__(self, *exc):
        global MIE_MEMO_ENTRIES, HG_FIT_MEMO_ENTRIES
        MIE_MEMO_ENTRIES, HG_FIT_MEMO_ENTRIES = self.saved
        return False


BRDF_MEMO_ENTRIES = 2                  # BRDF matrices the surface hook remembers: no model of the reference retrieves a Hapke
                                       # parameter, and one matrix is 0.18 GB at W = 10^4, NMU = 16, NF = 8
HAPKE_ATTRS = ("SGLALB", "K", "BS0", "hs", "BC0", "hc", "ROUGHNESS", "G1", "G2", "F")   # calc_Hapke_BRDF's order


def install_gpu_surface(device=0):
    """Route surface reflection through the GPU.

    The module-level Surface_0.calc_Hapke_BRDF (Surface_0.py:1292) and calc_OrenNayar_BRDF (:1743) are replaced: the class
    method Surface_0.calc_BRDF (:916) resolves them by global name at call time, which also routes the single-scattering
    branch's calc_BRDF(WAVE, SOL_ANG, EMISS_ANG, AZI_ANG) (ForwardModel_0.py:4307).  ForwardModel_0.calc_brdf_matrix
    (:5168) -- for LOWBC = HAPKE NMU^2 (NPHI + 1) BRDF evaluations per wavenumber and a four-deep interpreter loop over
    them -- becomes one engine call: the np.interp of the ten parameters onto WAVEC stays on the host, as in calc_BRDF
    (:952-961); every other LOWBC goes to the reference's method unchanged, which is no delegation.  The GPU forward-model
    class inherits the override.  The hook remembers the last BRDF_MEMO_ENTRIES matrices under the bytes of every argument
    and returns copies: the NX + 1 states of a staged Jacobian then cost one evaluation.  A call the engine refuses is
    delegated.  summary()["routes"] counts `brdf matrix`, `brdf matrix (memo)` and `brdf points`."""
    import importlib
    from collections import OrderedDict
    from ._lib import AnsfmError
    su = importlib.import_module("archnemesis.Surface_0")
    fm = importlib.import_module("archnemesis.ForwardModel_0")
    eng = get_engine(device)
    cls = fm.ForwardModel_0
    ref_hapke = getattr(su, "_ansfm_reference_calc_Hapke_BRDF", None) or su.calc_Hapke_BRDF
    ref_oren = getattr(su, "_ansfm_reference_calc_OrenNayar_BRDF", None) or su.calc_OrenNayar_BRDF
    ref_matrix = getattr(cls, "_ansfm_reference_calc_brdf_matrix", None) or cls.calc_brdf_matrix
    refused = (ValueError, NotImplementedError, AnsfmError)
    memo = OrderedDict()

    def calc_Hapke_BRDF(w, K, BS0, hs, BC0, hc, ROUGHNESS, G1, G2, F, i, e, phi):
        try:
            out = eng.surface_brdf(2, np.stack([np.asarray(a, dtype=np.float64) for a in (w, K, BS0, hs, BC0, hc, ROUGHNESS, G1, G2, F)]),
                                   i, e, phi)
        except refused:
            _delegate("calc_Hapke_BRDF: arguments the engine refuses")
            return ref_hapke(w, K, BS0, hs, BC0, hc, ROUGHNESS, G1, G2, F, i, e, phi)
        _route("brdf points")
        return out

    def calc_OrenNayar_BRDF(A, ROUGHNESS, i, e, phi):
        try:
            out = eng.surface_brdf(3, np.stack([np.asarray(a, dtype=np.float64) for a in (A, ROUGHNESS)]), i, e, phi)
        except refused:
            _delegate("calc_OrenNayar_BRDF: arguments the engine refuses")
            return ref_oren(A, ROUGHNESS, i, e, phi)
        _route("brdf points")
        return out

    def calc_brdf_matrix(self, WAVEC=None, Scatter=None, Surface=None):
        WAVEC = self.SpectroscopyX.WAVE if WAVEC is None else WAVEC
        Sc = self.ScatterX if Scatter is None else Scatter
        Su = self.SurfaceX if Surface is None else Surface
        if int(Su.LOWBC) != 2:
            return ref_matrix(self, WAVEC, Sc, Su)
        params = np.stack([np.interp(WAVEC, Su.VEM, getattr(Su, name)) for name in HAPKE_ATTRS])
        MU = np.ascontiguousarray(Sc.MU, dtype=np.float64)[:int(Sc.NMU)]
        key = (int(Sc.NPHI), int(Sc.NF), params.shape, params.tobytes(), MU.tobytes())
        hit = memo.get(key)
        if hit is not None:
            memo.move_to_end(key)
            _route("brdf matrix (memo)")
            return hit.copy()
        try:
            out = eng.brdf_matrix(2, params, MU, int(Sc.NPHI), int(Sc.NF))
        except refused:
            _delegate("calc_brdf_matrix: a quadrature the engine refuses")
            return ref_matrix(self, WAVEC, Sc, Su)
        _route("brdf matrix")
        memo[key] = np.array(out, dtype=np.float64)
        while len(memo) > BRDF_MEMO_ENTRIES:
            memo.popitem(last=False)
        return memo[key].copy()

    su._ansfm_reference_calc_Hapke_BRDF = ref_hapke
    su._ansfm_reference_calc_OrenNayar_BRDF = ref_oren
    cls._ansfm_reference_calc_brdf_matrix = ref_matrix
    su.calc_Hapke_BRDF = calc_Hapke_BRDF
    su.calc_OrenNayar_BRDF = calc_OrenNayar_BRDF
    cls.calc_brdf_matrix = calc_brdf_matrix
    return calc_brdf_matrix


def install_gpu_gradient_maps(device=0):
    """Route ForwardModel_0.map2pro / map2xvec (ForwardModel_0.py:5319, :5387) -- the layer -> profile -> state-vector
    gradient maps nemesisfmg applies right after CIRSrad(return_grad=True) (:704-711) -- through the GPU.  The arrays
    stay on the device between the three steps when they are passed on unmodified, as nemesisfmg does."""
    import importlib
    fm = importlib.import_module("archnemesis.ForwardModel_0")
    eng = get_engine(device)
    if not hasattr(fm, "_ansfm_reference_maps"):
        fm._ansfm_reference_maps = (fm.map2pro, fm.map2xvec)

    def map2pro(dSPECIN, NWAVE, NVMR, NDUST, NPRO, NPATH, NLAYIN, LAYINC, DTE, DAM, DCO, INCPAR=[-1]):
        return eng.map2pro(dSPECIN, NWAVE, NVMR, NDUST, NPRO, NPATH, NLAYIN, LAYINC, DTE, DAM, DCO, INCPAR=INCPAR)

    def map2xvec(dSPECIN, NWAVE, NVMR, NDUST, NPRO, NPATH, NX, xmap):
        return eng.map2xvec(dSPECIN, NWAVE, NVMR, NDUST, NPRO, NPATH, NX, xmap)

    fm.map2pro = map2pro
    fm.map2xvec = map2xvec
    return map2pro, map2xvec


def install_gpu_layering(device=0):
    """Route Layer_0.layer_average / layer_averageg (Layer_0.py:755, :1032; called by the Layer_0 methods of the same
    names, :509 / :552, from calc_path / calc_pathg) through the GPU."""
    import importlib
    l0 = importlib.import_module("archnemesis.Layer_0")
    eng = get_engine(device)
    if not hasattr(l0, "_ansfm_reference_layering"):
        l0._ansfm_reference_layering = (l0.layer_average, l0.layer_averageg)

    def _wrap(fn):
        def f(RADIUS, H, P, T, ID, VMR, DUST, PARAH2, BASEH, BASEP, LAYANG=0.0, LAYINT=0, LAYHT=0.0, NINT=101,
              DUST_UNITS=None, XMOLWT=None):
            r = list(fn(RADIUS, H, P, T, ID, VMR, DUST, PARAH2, BASEH, BASEP, LAYANG=LAYANG, LAYINT=int(LAYINT), LAYHT=LAYHT,
                        NINT=NINT, DUST_UNITS=DUST_UNITS, XMOLWT=XMOLWT))
            if np.ndim(VMR) == 1:                      # single-gas profiles come back 1-D in the reference
                r[4] = r[4][:, 0]; r[5] = r[5][:, 0]
            if DUST is not None and np.ndim(DUST) == 1:
                r[6] = r[6][:, 0]
            return tuple(r)
        return f

    l0.layer_average = _wrap(eng.layer_average)
    l0.layer_averageg = _wrap(eng.layer_averageg)
    return l0.layer_average, l0.layer_averageg


def install_gpu_convolution(device=0):
    """Route the ILS convolution kernels of Measurement_0 -- lblconv (:3335), lblconvg (:3799), lblconv_fil (:3549),
    lblconvg_fil (:3992), which the Measurement_0.lblconv / lblconvg methods call by module-global name with IGEOM = int
    (the way nemesisfm / nemesisfmg use them), and the *_ngeom variants (:3444, :3685, :3614, :3912; IGEOM = 'All') --
    through the GPU, and the filter-function branch of the k-table methods Measurement_0.conv / convg."""
    import importlib
    m0 = importlib.import_module("archnemesis.Measurement_0")
    eng = get_engine(device)
    if not hasattr(m0, "_ansfm_reference_conv"):
        m0._ansfm_reference_conv = (m0.lblconv, m0.lblconvg, m0.lblconv_fil, m0.lblconvg_fil, m0.lblconv_ngeom,
                                    m0.lblconvg_ngeom, m0.lblconv_fil_ngeom, m0.lblconvg_fil_ngeom)
    ref = m0._ansfm_reference_conv

    def _ascending(v):
        v = np.asarray(v)
        return v.ndim == 1 and np.all(v[1:] >= v[:-1])

    def lblconv(nwave, vwave, y, nconv, vconv, ishape, fwhm):
        if np.ndim(y) != 1 or not _ascending(vwave):
            _delegate("lblconv on an unsorted grid")
            return ref[0](nwave, vwave, y, nconv, vconv, ishape, fwhm)
        return eng.lblconv(nwave, vwave, y, nconv, vconv, int(ishape), fwhm)

    def lblconvg(nwave, vwave, y, dydx, nconv, vconv, ishape, fwhm):
        if np.ndim(y) != 1 or np.ndim(dydx) != 2 or not _ascending(vwave):
            _delegate("lblconvg on an unsorted grid")
            return ref[1](nwave, vwave, y, dydx, nconv, vconv, ishape, fwhm)
        return eng.lblconvg(nwave, vwave, y, dydx, nconv, vconv, int(ishape), fwhm)

    def lblconv_fil(nwave, vwave, y, nconv, vconv, nfil, vfil, afil):
        if np.ndim(y) != 1 or not _ascending(vwave):
            _delegate("lblconv_fil on an unsorted grid")
            return ref[2](nwave, vwave, y, nconv, vconv, nfil, vfil, afil)
        return eng.lblconv_fil(nwave, vwave, y, nconv, vconv, nfil, vfil, afil)

    def lblconvg_fil(nwave, vwave, y, dydx, nconv, vconv, nfil, vfil, afil):
        if np.ndim(y) != 1 or np.ndim(dydx) != 2 or not _ascending(vwave):
            _delegate("lblconvg_fil on an unsorted grid")
            return ref[3](nwave, vwave, y, dydx, nconv, vconv, nfil, vfil, afil)
        return eng.lblconvg_fil(nwave, vwave, y, dydx, nconv, vconv, nfil, vfil, afil)

    def lblconv_ngeom(nwave, vwave, y, nconv, vconv, ishape, fwhm):
        if np.ndim(y) != 2 or not _ascending(vwave) or not fwhm > 0.0:     # (the reference returns nothing for y.ndim != 2)
            _delegate("lblconv_ngeom on an unsorted grid")
            return ref[4](nwave, vwave, y, nconv, vconv, ishape, fwhm)
        return eng.lblconv_ngeom(nwave, vwave, y, nconv, vconv, int(ishape), fwhm)

    def lblconvg_ngeom(nwave, vwave, y, dydx, nconv, vconv, ishape, fwhm):
        if np.ndim(y) != 2 or np.ndim(dydx) != 3 or not _ascending(vwave) or not fwhm > 0.0:
            _delegate("lblconvg_ngeom on an unsorted grid")
            return ref[5](nwave, vwave, y, dydx, nconv, vconv, ishape, fwhm)
        return eng.lblconvg_ngeom(nwave, vwave, y, dydx, nconv, vconv, int(ishape), fwhm)

    def lblconv_fil_ngeom(nwave, vwave, y, nconv, vconv, nfil, vfil, afil):
        if np.ndim(y) != 2 or not _ascending(vwave):
            _delegate("lblconv_fil_ngeom on an unsorted grid")
            return ref[6](nwave, vwave, y, nconv, vconv, nfil, vfil, afil)
        return eng.lblconv_fil_ngeom(nwave, vwave, y, nconv, vconv, nfil, vfil, afil)

    def lblconvg_fil_ngeom(nwave, vwave, y, dydx, nconv, vconv, nfil, vfil, afil):
        if np.ndim(y) != 2 or np.ndim(dydx) != 3 or not _ascending(vwave):
            _delegate("lblconvg_fil_ngeom on an unsorted grid")
            return ref[7](nwave, vwave, y, dydx, nconv, vconv, nfil, vfil, afil)
        return eng.lblconvg_fil_ngeom(nwave, vwave, y, dydx, nconv, vconv, nfil, vfil, afil)

    # k-table runs: Measurement_0.conv (:2288) / convg (:2467).  Their FWHM < 0 branch (one filter per convolution point,
    # Python loops over NCONV x window with NX-vectors) goes to the GPU; FWHM == 0 (one scipy interp1d call) and the
    # cubic-spline FWHM > 0 branch of conv (convg raises there in the reference, :2611) are the reference's own host code.
    cls = m0.Measurement_0
    if not hasattr(cls, "_ansfm_reference_conv_methods"):
        cls._ansfm_reference_conv_methods = (cls.conv, cls.convg)
    rconv, rconvg = cls._ansfm_reference_conv_methods

    def _fil_case(self, Wave, IGEOM):
        return (not isinstance(IGEOM, str)) and self.FWHM < 0.0 and _ascending(Wave)

    def conv(self, Wave, ModSpec, IGEOM='All', FWHMEXIST=''):
        if not _fil_case(self, Wave, IGEOM):
            if self.FWHM != 0.0:
                _delegate("Measurement_0.conv outside the filter-function branch (FWHM > 0 spline, IGEOM='All')")
            return rconv(self, Wave, ModSpec, IGEOM=IGEOM, FWHMEXIST=FWHMEXIST)
        n = int(self.NCONV[IGEOM])
        return eng.conv_fil(Wave, np.asarray(ModSpec)[:len(Wave)], None, n, self.VCONV[:n, IGEOM], self.NFIL, self.VFIL, self.AFIL)

    def convg(self, Wave, ModSpec, ModGrad, IGEOM='All', FWHMEXIST=''):
        if not _fil_case(self, Wave, IGEOM):
            if self.FWHM != 0.0:
                _delegate("Measurement_0.convg outside the filter-function branch (FWHM > 0, IGEOM='All')")
            return rconvg(self, Wave, ModSpec, ModGrad, IGEOM=IGEOM, FWHMEXIST=FWHMEXIST)
        n = int(self.NCONV[IGEOM])
        return eng.conv_fil(Wave, np.asarray(ModSpec)[:len(Wave)], ModGrad, n, self.VCONV[:n, IGEOM], self.NFIL, self.VFIL,
                            self.AFIL)

    cls.conv, cls.convg = conv, convg
    # filter integrals (:4079-4300): np.trapz of filter x spectrum per convolution point
    if not hasattr(m0, "_ansfm_reference_intf"):
        m0._ansfm_reference_intf = (m0.integrate_filter, m0.integrate_filter_ngeom, m0.integrate_filterg, m0.integrate_filterg_ngeom)
    rint = m0._ansfm_reference_intf

    def _intf(k, nd, with_grad):
        def f(nwave, vwave, y, *rest):
            dydx = rest[0] if with_grad else None
            nconv, vconv, nfil, vfil, afil = rest[1:] if with_grad else rest
            if np.ndim(y) != nd or (with_grad and np.ndim(dydx) != nd + 1) or not _ascending(vwave):
                _delegate("integrate_filter* on an unsorted grid")
                return rint[k](nwave, vwave, y, *rest)
            return eng.integrate_filter(nwave, vwave, y, nconv, vconv, nfil, vfil, afil, dydx=dydx)
        return f

    m0.integrate_filter, m0.integrate_filter_ngeom = _intf(0, 1, False), _intf(1, 2, False)
    m0.integrate_filterg, m0.integrate_filterg_ngeom = _intf(2, 1, True), _intf(3, 2, True)
    m0.lblconv, m0.lblconvg, m0.lblconv_fil, m0.lblconvg_fil = lblconv, lblconvg, lblconv_fil, lblconvg_fil
    m0.lblconv_ngeom, m0.lblconvg_ngeom = lblconv_ngeom, lblconvg_ngeom
    m0.lblconv_fil_ngeom, m0.lblconvg_fil_ngeom = lblconv_fil_ngeom, lblconvg_fil_ngeom
    return lblconv, lblconvg, lblconv_fil, lblconvg_fil


def install_gpu_continuum(device=0):
    """Route ForwardModel_0.calc_tau_cia (ForwardModel_0.py:4516) -- per forward model ~2 scipy interp1d constructions per
    (layer, CIA pair) on the host --, calc_tau_rayleigh (:4869) and calc_tau_dust (:4790) through the GPU.  The wavenumber-only parametrisations co2cia / n2n2cia / n2h2cia
    (CIA_0.py:631-880, embedded data tables) are still evaluated by the reference's own functions and passed as vectors."""
    import importlib
    fm = importlib.import_module("archnemesis.ForwardModel_0")
    cm = importlib.import_module("archnemesis.CIA_0")
    eng = get_engine(device)
    cls = fm.ForwardModel_0
    ref = getattr(cls, "_ansfm_reference_calc_tau_cia", None) or cls.calc_tau_cia

    def calc_tau_cia(self, ISPACE=None, WAVEC=None, CIA=None, Atmosphere=None, Layer=None, MakePlot=False):
        if MakePlot:
            _delegate("calc_tau_cia(MakePlot=True)")
            return ref(self, ISPACE, WAVEC, CIA, Atmosphere, Layer, MakePlot)
        ISPACE = int(self.MeasurementX.ISPACE) if ISPACE is None else int(ISPACE)
        WAVEC = self.SpectroscopyX.WAVE if WAVEC is None else WAVEC
        CIA = self.CIAX if CIA is None else CIA
        A = self.AtmosphereX if Atmosphere is None else Atmosphere
        L = self.LayerX if Layer is None else Layer
        WAVEC = np.asarray(WAVEC, dtype=np.float64)
        WAVEN = WAVEC if ISPACE == 0 else np.sort(1.e4 / WAVEC)
        ID = np.asarray(A.ID); ISO = np.asarray(A.ISO)
        has = lambda gid: np.any((ID == gid))
        return eng.calc_tau_cia(ISPACE, WAVEC, CIA.WAVEN, CIA.TEMP, CIA.FRAC, int(CIA.NPARA), CIA.K_CIA,
                                [int(g) for g in CIA.IPAIRG1], [int(g) for g in CIA.IPAIRG2], [int(g) for g in CIA.INORMALT],
                                int(CIA.INORMAL), CIA.locate_INORMAL_pairs(), ID, ISO, L.PP, L.PRESS, L.TEMP, L.FRAC, L.TOTAM, L.DELH,
                                k_co2=cm.co2cia(WAVEN) if has(2) else None, k_n2n2=cm.n2n2cia(WAVEN) if has(22) else None,
                                k_n2h2=cm.n2h2cia(WAVEN) if (has(22) and has(39)) else None)

    cls._ansfm_reference_calc_tau_cia = ref
    cls.calc_tau_cia = calc_tau_cia

    # Rayleigh scattering (:4869) and aerosols (:4790): same pattern, the reference's methods keep their signatures
    ref_ray = getattr(cls, "_ansfm_reference_calc_tau_rayleigh", None) or cls.calc_tau_rayleigh
    ref_dust = getattr(cls, "_ansfm_reference_calc_tau_dust", None) or cls.calc_tau_dust

    def calc_tau_rayleigh(self, IRAY=None, ISPACE=None, WAVEC=None, ID=None, ISO=None, Layer=None, MakePlot=False):
        if MakePlot:
            _delegate("calc_tau_rayleigh(MakePlot=True)")
            return ref_ray(self, IRAY, ISPACE, WAVEC, ID, ISO, Layer, MakePlot)
        IRAY = int(self.ScatterX.IRAY if IRAY is None else IRAY)
        ISPACE = int(self.MeasurementX.ISPACE if ISPACE is None else ISPACE)
        WAVEC = self.SpectroscopyX.WAVE if WAVEC is None else WAVEC
        ID = self.AtmosphereX.ID if ID is None else ID
        ISO = self.AtmosphereX.ISO if ISO is None else ISO
        L = self.LayerX if Layer is None else Layer
        VMR = (np.asarray(L.PP).T / np.asarray(L.PRESS)).T if IRAY == 4 else None
        return eng.calc_tau_rayleigh(IRAY, ISPACE, WAVEC, L.TOTAM, ID, ISO, VMR)

    def calc_tau_dust(self, WAVEC=None, Scatter=None, Layer=None, MakePlot=False):
        WAVEC = self.SpectroscopyX.WAVE if WAVEC is None else WAVEC
        S = self.ScatterX if Scatter is None else Scatter
        L = self.LayerX if Layer is None else Layer
        WAVEC = np.asarray(WAVEC, dtype=np.float64)
        if self.Scatter.NDUST > 0:                                      # the reference's own range test (:4819-4823)
            if (WAVEC.min() < S.WAVE.min()) & (WAVEC.max() > S.WAVE.min()):
                raise ValueError('error calc_tau_dust :: Spectral range for calculation is outside of range in which the Aerosol properties are defined')
        for i in range(S.NDUST):                                        # side effect on Layer.CONT kept (:4833-4834)
            if i in self.AtmosphereX.DUST_RENORMALISATION.keys():
                L.CONT[:, i] = L.CONT[:, i] / L.CONT[:, i].sum() * 1e4 * self.AtmosphereX.DUST_RENORMALISATION[i]
        if S.NDUST == 0:
            z = np.zeros((len(WAVEC), L.NLAY, 0))
            return z, z.copy(), z.copy(), z.copy()
        return eng.calc_tau_dust(WAVEC, S.WAVE, np.asarray(S.KEXT)[:, :S.NDUST], np.asarray(S.KSCA)[:, :S.NDUST],
                                 np.asarray(L.CONT)[:, :S.NDUST])

    cls._ansfm_reference_calc_tau_rayleigh = ref_ray
    cls._ansfm_reference_calc_tau_dust = ref_dust
    cls.calc_tau_rayleigh = calc_tau_rayleigh
    cls.calc_tau_dust = calc_tau_dust
    return calc_tau_cia


def install_gpu_table_reader(device=0):
    """Spectroscopy_0.read_tables (Spectroscopy_0.py:1448) for binary k-tables (.kta) and LBL tables (.lta, ILBL = 2;
    read_lbltable :2626 loops over (wavenumber, pressure) in Python) without the host array: the header logic
    (read_header, the searchsorted cut of WAVE to [wavemin, wavemax], :1482-1494) is the reference's, but instead of
    unpacking every table with the Python loops of read_ktable (:2846-2850) into a float64 (NWAVE,NG,NP,NT,NGAS) array,
    Spectroscopy.K becomes a KtaTableOnDevice description and the GPU CIRSrad streams the files into HBM
    (ansfm_upload_ktable_files) -- once, since nemesisfm re-reads the tables for every forward model (:480-482) and the
    fingerprint of unchanged files matches.  Other table kinds go to the reference's read_tables."""
    import importlib
    sp = importlib.import_module("archnemesis.Spectroscopy_0")
    cls = sp.Spectroscopy_0
    ref = getattr(cls, "_ansfm_reference_read_tables", None) or cls.read_tables

    def read_tables(self, wavemin=0., wavemax=1.0e10, wavedelta=1.0):
        ext = {ILBL_K_TABLES: "kta", ILBL_LBL_TABLES: "lta"}.get(int(self.ILBL))
        binary = (ext is not None and self.LOCATION is not None and not getattr(self, "ONLINE", False)
                  and len(self.LOCATION) > 0 and all(str(p).endswith(ext) for p in self.LOCATION))
        if not binary:
            _delegate("read_tables for tables that are not binary .kta / .lta files")
            return ref(self, wavemin, wavemax, wavedelta)
        if self.WAVE is None:
            self.read_header()
        iwl = np.searchsorted(self.WAVE, wavemin, side='right') - 1      # :1486-1494
        if iwl < 0:
            iwl = 0
        iwh = np.searchsorted(self.WAVE, wavemax, side='left')
        if iwh >= self.NWAVE:
            iwh = self.NWAVE - 1
        wave1 = self.WAVE[iwl:iwh + 1]
        self.NWAVE = len(wave1)
        self.WAVE = wave1
        if ext == "lta":
            self.K = KtaTableOnDevice(self.LOCATION, self.WAVE.min(), self.WAVE.max(),       # NT < 0: |NT| temperatures per level
                                      (self.NWAVE, self.NP, abs(int(self.NT)), self.NGAS), sp.read_lbltable, ".lta", 8)
        else:
            self.K = KtaTableOnDevice(self.LOCATION, self.WAVE.min(), self.WAVE.max(),
                                      (self.NWAVE, self.NG, self.NP, self.NT, self.NGAS), sp.read_ktable)

    cls._ansfm_reference_read_tables = ref
    cls.read_tables = read_tables
    return read_tables


class Installed(list):
    """What install_all() returns: the names installed, and `summary()` -- every case that left the GPU path since then
    (DELEGATED: case -> count; each is also announced once as a RuntimeWarning) and every deliberate difference (NOTES)."""

    @staticmethod
    def summary():
        return summary()

    def __repr__(self):
        s = summary()
        return "Installed(%s; delegated to the reference so far: %s; notes: %s)" % (list.__repr__(self), s["delegated"] or "nothing",
                                                                                     s["notes"] or "none")


def install_all(device=0, oe_linalg=True, ktable_generator=True, forward_model=True):
    """Every replacement this package has for the imported reference, in one call; returns the
    names installed as an `Installed` list whose `summary()` reports what was handed to the reference's CPU code since.
    forward_model=True also makes `archnemesis.ForwardModel_0` name the GPU subclass (install_gpu_forward_model), so that
    `coreretOE` / `retrieval_nemesis` build it."""
    done = Installed()
    if forward_model:
        install_gpu_forward_model(device); done.append("install_gpu_forward_model")
    for f in (install_gpu_gradient_maps, install_gpu_scattering_core, install_gpu_line_kernel, install_gpu_pseudo_continuum,
              install_gpu_mie, install_gpu_hg_fit, install_gpu_surface, install_gpu_layering, install_gpu_convolution, install_gpu_continuum,
              install_gpu_table_reader):
        f(device); done.append(f.__name__)
    if oe_linalg:
        from .oe_linalg import install_gpu_oe_linalg
        install_gpu_oe_linalg(device); done.append("install_gpu_oe_linalg")
    if ktable_generator:
        from .ktable_gen import install_gpu_ktable_generator
        install_gpu_ktable_generator(device); done.append("install_gpu_ktable_generator")
    return done
