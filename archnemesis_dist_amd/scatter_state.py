"""State vector <-> atmosphere <-> multiple-scattering spectra for a batch of states: profile_state's route for the scattering
branch of CIRSrad (ForwardModel_0.py:4478-4501, scloud11wave :5018-5165), so that a numerical Jacobian of a scattering
configuration is one batched call too.

    state vector  --model 0-->  T, VMR, aerosol profiles at the levels                  host, a few kB per state
                  --layer_average (Curtis-Godson)-->  layers of every state               k_layer_average (one launch, all states)
                  --CIA, aerosol extinction / scattering / fractions, Rayleigh-->         k_ms_cont_rows inside the CIRSrad call,
                                                                                          per distinct layer, from resident sources
                  --calc_k + k_overlap, doubling / adding, g-quadrature-->                the batched scattering branch with its
                                                                                          layer cache (cirsrad_ck_scatter_batch_cont)
Supported: ILBL = K_TABLES, continuous-profile variables (temperature, ln VMR, ln aerosol profile), the phase functions as
tabulated arrays (no subfithgm / legfit), no hydrostatic re-adjustment, no instrument convolution, at most 7 aerosol
populations, no DUST_RENORMALISATION-style rescaling of the aerosol columns.
"""
import numpy as np

from . import layering
from .continuum_rows import ContinuumRows

SQ_CM_TO_SQ_METER = 1.0e-4       # ForwardModel_0.py:66
MAX_POPULATIONS = 7              # NumPy sums 8 and more populations pairwise; the kernels sum in order (ansfm_upload_dust)


def planck(ISPACE, WAVE, T):
    """planck_wave (ForwardModel_0.py:6214-6215): WAVE wavenumbers (ISPACE 0) or wavelengths in micron -> radiance at T"""
    c1, c2 = 1.1911e-12, 1.439
    WAVE = np.asarray(WAVE, float)
    if int(ISPACE) == 0:
        y = WAVE; a = c1 * y ** 3
    else:
        y = 1.0e4 / WAVE; a = c1 * y ** 5 / 1.0e4
    return a / (np.exp(c2 * y / T) - 1.0)


def continuum_rows_by_hand(eng, ISPACE, IRAY, ID, ISO, cia, dust, lay):
    """The continuum of n states at array level, packed once per distinct layer: calc_tau_cia / calc_tau_dust over all n * L
    layers, calc_tau_rayleigh_batch_dev, the sums and fractions of calculate_layer_opacity (:3966-3972) and scloud11wave
    (:5107-5113), then ContinuumRows -- the route `BatchedCKScatterModel.fused_continuum` replaces, from entries that do not
    know the fused one.  cia: dict of calc_tau_cia's table arguments by name (k_co2 / k_n2n2 / k_n2h2 on the table's grid) or
    None; dust: dict(SWAVE, KEXT, KSCA) or None; lay: host arrays PP, PRESS, TEMP, FRAC, TOTAM, DELH, CONT with the state axis
    first.  -> ContinuumRows of the n states."""
    import torch
    n, L = lay["PRESS"].shape
    WAVE = eng.WAVE
    W = WAVE.size
    flat = lambda a: np.ascontiguousarray(a).reshape((n * L,) + np.shape(a)[2:])
    per_state = lambda a: np.ascontiguousarray(np.moveaxis(np.asarray(a).reshape((W, n, L) + np.shape(a)[2:]), 1, 0))
    TAUCIA = TAUDUST = TAURAY = TAUSCAT = FRAC = None
    if cia is not None:
        k = {}
        for name in ("k_co2", "k_n2n2", "k_n2h2"):                # calc_tau_cia takes them in its own (sorted) order
            v = cia.get(name)
            k[name] = None if v is None else (np.asarray(v, float) if int(ISPACE) == 0 else
                                              np.asarray(v, float)[np.argsort(1.e4 / WAVE)])
        tau = eng.calc_tau_cia(ISPACE, WAVE, cia["CIA_WAVEN"], cia["CIA_TEMP"], cia["CIA_FRAC"], cia["NPARA"], cia["K_CIA"],
                               cia["IPAIRG1"], cia["IPAIRG2"], cia["INORMALT"], cia["INORMAL"], cia["INORMALD"], ID, ISO,
                               flat(lay["PP"]), flat(lay["PRESS"]), flat(lay["TEMP"]), flat(lay["FRAC"]), flat(lay["TOTAM"]),
                               flat(lay["DELH"]), with_grad=False, **k)
        TAUCIA = per_state(tau)                                    # (n, W, L)
    if dust is not None:
        td1, tcs = eng.calc_tau_dust(WAVE, dust["SWAVE"], dust["KEXT"], dust["KSCA"], flat(lay["CONT"]))[:2]     # (W, n L, NDUST)
        td1 = np.clip(np.nan_to_num(td1), 0, 1e20)                 # :3966
        dsum, ssum = np.sum(td1, 2), np.sum(tcs, 2)                # :3971-3972
        frac = np.zeros_like(tcs)                                  # :5107-5113
        ii = np.where(ssum > 0.0)
        if ii[0].size > 0:
            frac[ii[0], ii[1], :] = (tcs[ii[0], ii[1], :].T / ssum[ii[0], ii[1]]).T
        TAUDUST, TAUSCAT = per_state(dsum), per_state(ssum)
        FRAC = np.ascontiguousarray(np.transpose(per_state(frac), (0, 1, 3, 2)))            # (n, W, NDUST, L)
    if int(IRAY) != 0:
        dev = torch.device("cuda", eng.device)
        ray = torch.empty((n, W, L), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        eng.calc_tau_rayleigh_batch_dev(IRAY, ISPACE, np.ascontiguousarray(lay["TOTAM"]), ray, ID=ID, ISO=ISO,
                                        VMR=lay["PP"] / lay["PRESS"][:, :, None])
        eng.synchronize()
        TAURAY = ray.cpu().numpy()
    pk = ContinuumRows(L, 0 if FRAC is None else FRAC.shape[2])
    at = lambda a, m: None if a is None else a[m]
    for m in range(n):
        pk.add_state(at(TAUCIA, m), at(TAUDUST, m), at(TAURAY, m), at(TAUSCAT, m), at(FRAC, m))
    return pk


def _phase_source(what, phase_source, dense, dust):
    """phase_source=(imie, THETA_TAB, tab) of a model -> (imie, THETA_TAB float64, tab float64), or None; it stands in for the
    dense host array and lives on the aerosol grid dust["SWAVE"]"""
    if phase_source is None:
        return None
    if dense is not None or dust is None:
        raise ValueError(what + "phase_source replaces the dense phase-function array (pass None) and needs dust=dict(SWAVE, KEXT, KSCA)")
    imie, theta, tab = phase_source
    tab = np.ascontiguousarray(tab, dtype=float)
    if tab.ndim != 3:
        raise ValueError(what + "phase_source = (imie, THETA_TAB, tab), tab as AnsfmEngine.calc_phase takes it")
    return int(imie), (None if theta is None else np.ascontiguousarray(theta, dtype=float)), tab


class BatchedCKScatterModel:
    """The scattering forward model of n states at once (see the module docstring); what `jacobian.jacobian_nemesis_batched`
    asks of a model.

    eng: AnsfmEngine with the k-table uploaded.  state: ContinuousProfileState, with or without a ("DUST", column) block.
    ID / ISO, igas_map, layering_args, ISPACE, IRAY, PARAH2, cia: as profile_state.BatchedCKThermalModel takes them.
    dust: dict(SWAVE, KEXT, KSCA (NWAVE_scatter, NDUST)[, DUST (NPRO, NDUST)]) -- the aerosol profiles are the state's when it
    has a DUST block, else dust["DUST"], the same for every state.
    phasarr (NDUST, NWAVE, 2, NTHETA) as the engine takes it, MU / WTMU the quadrature, NF, NPHI, IMIE; SOL_ANG / EMISS_ANG /
    AZI_ANG: lists, one entry per geometry; solar (NWAVE); LOWBC and brdf_matrix (NWAVE, NMU, NMU, NF + 1; None: zeros);
    TSURF, emissivity (NWAVE; None: 1) and gasgiant decide the boundary radiance (:5083-5089).
    phase_source=(imie, THETA, tab) instead of phasarr (pass None): the phase function as a resident source of the engine
    (upload_phase on dust["SWAVE"], uploaded with the aerosol source; tab as AnsfmEngine.calc_phase takes it, THETA =
    Scatter.THETA) and phasarr formed on the device (cirsrad_ck_scatter_batch_src).  Whole axis only.
    DUST_RENORMALISATION: the reference rescales the aerosol columns in the caller of calc_tau_dust; anything but None / False
    raises NotImplementedError, as do more than 7 populations."""

    fused_continuum = True    # False: the continuum of all n * NLAY layers at array level, packed by ContinuumRows, through
                              # cirsrad_ck_scatter_batch_rows (same bits)

    def __init__(self, eng, state, RADIUS, ID, ISO, igas_map, phasarr, MU, WTMU, NF, NPHI, SOL_ANG, EMISS_ANG, AZI_ANG, solar,
                 layering_args=None, ISPACE=0, IRAY=0, IMIE=0, PARAH2=None, cia=None, dust=None, LOWBC=0, brdf_matrix=None,
                 TSURF=-1.0, emissivity=None, gasgiant=True, DUST_RENORMALISATION=None, phase_source=None):
        if DUST_RENORMALISATION is not None and DUST_RENORMALISATION is not False:
            raise NotImplementedError("BatchedCKScatterModel: DUST_RENORMALISATION-style rescaling of the aerosol columns is applied "
                                      "by the caller of calc_tau_dust in the reference and is not built here")
        self.dust = None if dust is None else dict(dust)
        DUST = state.DUST if getattr(state, "has_dust", False) else (None if self.dust is None else self.dust.get("DUST"))
        if getattr(state, "has_dust", False) and self.dust is None:
            raise ValueError("BatchedCKScatterModel: a state with a DUST block needs dust=dict(SWAVE, KEXT, KSCA)")
        if self.dust is not None:
            if DUST is None:
                raise ValueError("BatchedCKScatterModel: no aerosol profiles (a DUST block of the state, or dust['DUST'])")
            DUST = np.asarray(DUST, float).reshape(state.NPRO, -1)
            if max(DUST.shape[1], np.shape(self.dust["KEXT"])[1]) > MAX_POPULATIONS:
                raise NotImplementedError("BatchedCKScatterModel: more than 7 aerosol populations (NumPy sums 8 and more pairwise, "
                                          "the kernels sum in order)")
            if DUST.shape[1] != np.shape(self.dust["KEXT"])[1] or np.shape(self.dust["KSCA"]) != np.shape(self.dust["KEXT"]):
                raise ValueError("BatchedCKScatterModel: KEXT / KSCA (NWAVE_scatter, NDUST) and DUST (NPRO, NDUST) disagree")
        self.DUST = DUST
        self.eng, self.state = eng, state
        self.RADIUS = float(RADIUS)
        self.ID = np.asarray(ID); self.ISO = np.asarray(ISO)
        self.igas_map = np.asarray(igas_map, dtype=np.int64)
        la = dict(NLAY=20, LAYTYP=layering.EQUAL_LOG_PRESSURE, LAYINT=1, LAYHT=0.0, LAYANG=0.0, NINT=101)
        la.update(layering_args or {})
        self.lay = la
        self.ISPACE, self.IRAY, self.IMIE = int(ISPACE), int(IRAY), int(IMIE)
        self.cia = None if cia is None else dict(cia)
        self.PARAH2 = PARAH2
        self.MU, self.WTMU = np.asarray(MU, float), np.asarray(WTMU, float)
        self.NF, self.NPHI, self.LOWBC = int(NF), int(NPHI), int(LOWBC)
        self.SOL_ANG, self.EMISS_ANG, self.AZI_ANG = (np.atleast_1d(np.asarray(a, float)) for a in (SOL_ANG, EMISS_ANG, AZI_ANG))
        if not (self.SOL_ANG.size == self.EMISS_ANG.size == self.AZI_ANG.size):
            raise ValueError("BatchedCKScatterModel: SOL_ANG, EMISS_ANG and AZI_ANG list one entry per geometry")
        self.TSURF, self.gasgiant = float(TSURF), bool(gasgiant)
        dims, _ = eng.ktable_info()
        self.W = int(dims[0])
        NMU = self.MU.size
        self.phasarr = None if phasarr is None else np.ascontiguousarray(phasarr, dtype=float)
        ncont = 0 if self.phasarr is None else self.phasarr.shape[0]
        self.phase_source = _phase_source("BatchedCKScatterModel: ", phase_source, self.phasarr, self.dust)
        if self.phase_source is not None:
            ncont = self.phase_source[2].shape[2]
            if self.phase_source[1] is None or self.phase_source[1].size < 3:
                raise ValueError("BatchedCKScatterModel: phase_source needs Scatter.THETA, at least three angles")
            if (self.phase_source[0] == 0) != (self.IMIE == 0):
                raise ValueError("BatchedCKScatterModel: phase_source and IMIE disagree about Henyey-Greenstein phase functions")
        if ncont != (0 if self.DUST is None else self.DUST.shape[1]):
            raise ValueError("BatchedCKScatterModel: phasarr (NDUST, NWAVE, 2, NTHETA) lists one phase function per population")
        self.solar = np.ascontiguousarray(solar, dtype=float)
        self.emissivity = np.ones(self.W) if emissivity is None else np.ascontiguousarray(emissivity, dtype=float)
        self.brdf_matrix = (np.zeros((self.W, NMU, NMU, self.NF + 1)) if brdf_matrix is None
                            else np.ascontiguousarray(brdf_matrix, dtype=float))
        self.BASEH, self.BASEP = layering.layer_split(self.RADIUS, state.H, state.P, LAYANG=la["LAYANG"], LAYHT=la["LAYHT"],
                                                      NLAY=la["NLAY"], LAYTYP=la["LAYTYP"])
        self._sources_on = False
        self.last_rows = (0, 0)       # opacity rows computed / (state, layer) pairs, last spectra_batch
        self.last_cache = (0, 0)      # layers taken from the first state's doubling results / layers of the other states

    # ---- what jacobian_nemesis_batched asks of a model -------------------------------------------------------------
    def ny(self):
        """length of a measurement vector of this model (its wavenumbers x geometries)"""
        return self.W * self.EMISS_ANG.size

    def torch_device(self):
        import torch
        return torch.device("cuda", self.eng.device)

    # ---- host part: the profiles and layers of n states -----------------------------------------------------------
    def layers(self, X):
        """X (n, NX) -> dict of per-state layer arrays (Layer_0 attributes after calc_layering), the aerosol columns CONT of
        every state's own aerosol profiles among them, `amount` (n, NGAS, NLAY) of the table's gases and VMRLAY."""
        st, la = self.state, self.lay
        prof = st.profiles(X)
        T, VMR = prof[0], prof[1]
        n = T.shape[0]
        DUST = prof[2] if len(prof) > 2 else (None if self.DUST is None else np.repeat(self.DUST[None], n, 0))
        H = np.repeat(st.H[None], n, 0); P = np.repeat(st.P[None], n, 0)
        PARAH2 = (self.PARAH2 if self.PARAH2 is None or np.ndim(self.PARAH2) != 1
                  else np.repeat(np.asarray(self.PARAH2, float)[None], n, 0))
        out = self.eng.layer_average(self.RADIUS, H, P, T, self.ID, VMR, DUST, PARAH2, self.BASEH, self.BASEP,
                                     LAYANG=la["LAYANG"], LAYINT=la["LAYINT"], LAYHT=la["LAYHT"], NINT=la["NINT"])
        names = ("HEIGHT", "PRESS", "TEMP", "TOTAM", "AMOUNT", "PP", "CONT", "FRAC", "DELH", "BASET", "LAYSF")
        lay = dict(zip(names, out))
        lay["amount"] = np.ascontiguousarray(np.transpose(lay["AMOUNT"][:, :, self.igas_map], (0, 2, 1))) * SQ_CM_TO_SQ_METER
        lay["VMRLAY"] = lay["PP"] / lay["PRESS"][:, :, None]
        return lay

    def radg(self, lay):
        """the boundary radiance of every state, (n, NWAVE, NMU): Planck at the bottom layer's temperature for a gas giant or
        TSURF <= 0, else B(TSURF) * emissivity (:5083-5089)"""
        WAVE, NMU = self.eng.WAVE, self.MU.size
        n = lay["TEMP"].shape[0]
        if self.gasgiant or self.TSURF <= 0.0:
            rg = np.stack([planck(self.ISPACE, WAVE, lay["TEMP"][m, 0]) for m in range(n)])
        else:
            rg = np.repeat((planck(self.ISPACE, WAVE, self.TSURF) * self.emissivity)[None], n, 0)
        return np.ascontiguousarray(np.repeat(rg[:, :, None], NMU, 2))

    def upload_sources(self):
        """Make `cia` / `dust` resident sources of the engine, on the grid of the table it holds now."""
        eng = self.eng
        if self.cia is not None:
            c = self.cia
            eng.upload_cia(self.ISPACE, None, c["CIA_WAVEN"], c["CIA_TEMP"], c["CIA_FRAC"], c["NPARA"], c["K_CIA"], c["IPAIRG1"],
                           c["IPAIRG2"], c["INORMALT"], c["INORMAL"], c["INORMALD"], self.ID, self.ISO, k_co2=c.get("k_co2"),
                           k_n2n2=c.get("k_n2n2"), k_n2h2=c.get("k_n2h2"))
        if self.dust is not None:
            eng.upload_dust(self.dust["SWAVE"], self.dust["KEXT"], self.dust["KSCA"])
        if self.phase_source is not None:
            eng.upload_phase(self.phase_source[0], self.dust["SWAVE"], self.phase_source[1], self.phase_source[2])
        self._sources_on = True

    # ---- device part ----------------------------------------------------------------------------------------------
    def spectra_batch(self, X, device=None, wave_slice=None):
        """Spectra of the n states X (n, NX): torch tensor (n, NY), NY = NWAVE * NGEOM (geometry fastest like SPECOUT), on the
        engine's device.  wave_slice = (w_begin, W_full): the engine's table is that slice of a longer axis; phasarr then
        covers all of it, every other per-wavenumber input of the model the slice."""
        import torch
        eng = self.eng
        dev = torch.device("cuda", eng.device) if device is None else device
        lay = self.layers(X)
        n, L = lay["PRESS"].shape
        cia, dust = self.cia is not None, self.dust is not None
        src = self.phase_source
        if src is not None and not (self.fused_continuum and wave_slice is None):
            raise NotImplementedError("BatchedCKScatterModel: phase_source needs the fused continuum and the whole spectral axis")
        common = (self.phasarr if src is None else src[1], self.radg(lay), self.SOL_ANG, self.EMISS_ANG, self.AZI_ANG, self.solar, self.LOWBC, self.brdf_matrix,
                  self.MU, self.WTMU, self.NF, self.NPHI, self.IRAY, self.IMIE)
        if self.fused_continuum and (cia or dust or self.IRAY != 0):
            if not self._sources_on:
                self.upload_sources()
            f4 = eng.rayleigh_f4(self.ID, self.ISO, lay["VMRLAY"]) if self.IRAY == 4 else None
            entry = eng.cirsrad_ck_scatter_batch_cont if src is None else eng.cirsrad_ck_scatter_batch_src
            out = entry(self.ISPACE, lay["PRESS"], lay["TEMP"], lay["amount"], lay["VMRLAY"] if cia else None,
                        lay["FRAC"] if cia else None, lay["TOTAM"], lay["DELH"] if cia else None, lay["CONT"] if dust else None,
                        self.IRAY, f4, *common, wave_slice=wave_slice)
        else:
            pk = continuum_rows_by_hand(eng, self.ISPACE, self.IRAY, self.ID, self.ISO, self.cia, self.dust, lay)
            out = eng.cirsrad_ck_scatter_batch_rows(self.ISPACE, lay["PRESS"], lay["TEMP"], lay["amount"], pk.cont_row,
                                                    pk.TAUCIA_rows, pk.TAUDUST_rows, pk.TAURAY_rows, pk.TAUSCAT_rows, self.phasarr,
                                                    pk.lfrac_rows, *common[1:], wave_slice=wave_slice)
        self.last_rows = eng.last_layer_rows()
        self.last_cache = eng.last_scatter_cache()
        return torch.as_tensor(out.reshape(n, -1), dtype=torch.float64, device=dev)


# ---- the single-scattering branch -----------------------------------------------------------------------------------------
def singlescatt_phase_and_sca(TAUCLSCAT, TAURAY, TAUSCAT, phase_fn):
    """The layer-mean phase function of every path and the scattering opacity of one state as
    calculate_single_scattering_plane_parallel_spectrum forms them (ForwardModel_0.py:4316-4321): TAUCLSCAT (NWAVE, NLAY,
    NDUST), TAURAY / TAUSCAT (NWAVE, NLAY), phase_fn (NWAVE, NPATH, NDUST + 1) -> tausca (NWAVE, NLAY), phase (NPATH, NWAVE,
    NLAY)."""
    W, L, ND = TAUCLSCAT.shape
    phase_function = np.transpose(np.asarray(phase_fn, float), (0, 2, 1))            # (NWAVE, NDUST + 1, NPATH), :4272
    P = phase_function.shape[2]
    out = np.zeros((P, W, L))
    for ipath in range(P):
        phasex = np.zeros((W, ND + 1, L))
        phasex[:, 0:ND, :] = np.transpose(phase_function[:, 0:ND, ipath] * np.transpose(TAUCLSCAT, axes=(1, 0, 2)), axes=(1, 2, 0))
        phasex[:, ND, :] = np.transpose(phase_function[:, ND, ipath] * np.transpose(TAURAY))
        phase = np.sum(phasex, axis=1)
        phase[phase > 0] = phase[phase > 0] / (TAURAY[phase > 0] + TAUSCAT[phase > 0])
        out[ipath] = phase
    return TAURAY + TAUSCAT, out


def singlescatt_dense_by_hand(eng, ISPACE, IRAY, ID, ISO, cia, dust, lay, phase_fn):
    """taucont, tausca (n, NWAVE, NLAY) and phase (n, NPATH, NWAVE, NLAY) of n states at array level: calc_tau_cia / calc_tau_dust
    / calc_tau_rayleigh over all n * L layers, the sums of calculate_layer_opacity (:3963-3989) and `singlescatt_phase_and_sca`
    per state -- the route `BatchedCKSingleScatterModel.fused_continuum` replaces.  cia, dust, lay as `continuum_rows_by_hand`
    takes them; a term that is not used is the reference's array of zeros."""
    n, L = lay["PRESS"].shape
    WAVE = eng.WAVE
    W = WAVE.size
    flat = lambda a: np.ascontiguousarray(a).reshape((n * L,) + np.shape(a)[2:])
    cont = None
    if cia is not None:
        k = {}
        for name in ("k_co2", "k_n2n2", "k_n2h2"):                # calc_tau_cia takes them in its own (sorted) order
            v = cia.get(name)
            k[name] = None if v is None else (np.asarray(v, float) if int(ISPACE) == 0 else
                                              np.asarray(v, float)[np.argsort(1.e4 / WAVE)])
        cont = eng.calc_tau_cia(ISPACE, WAVE, cia["CIA_WAVEN"], cia["CIA_TEMP"], cia["CIA_FRAC"], cia["NPARA"], cia["K_CIA"],
                                cia["IPAIRG1"], cia["IPAIRG2"], cia["INORMALT"], cia["INORMAL"], cia["INORMALD"], ID, ISO,
                                flat(lay["PP"]), flat(lay["PRESS"]), flat(lay["TEMP"]), flat(lay["FRAC"]), flat(lay["TOTAM"]),
                                flat(lay["DELH"]), with_grad=False, **k)                                   # (W, n L)
    TAUCLSCAT, TAUSCAT = np.zeros((W, n * L, 0)), np.zeros((W, n * L))
    if dust is not None:
        td1, TAUCLSCAT = eng.calc_tau_dust(WAVE, dust["SWAVE"], dust["KEXT"], dust["KSCA"], flat(lay["CONT"]))[:2]
        TAUDUST = np.sum(np.clip(np.nan_to_num(td1), 0, 1e20), 2)                                          # :3966, :3971
        TAUSCAT = np.sum(TAUCLSCAT, 2)                                                                     # :3972
        cont = TAUDUST if cont is None else cont + TAUDUST
    TAURAY = np.zeros((W, n * L))
    if int(IRAY) != 0:
        TAURAY = eng.calc_tau_rayleigh(IRAY, ISPACE, WAVE, flat(lay["TOTAM"]), ID=ID, ISO=ISO,
                                       VMR=flat(lay["PP"] / lay["PRESS"][:, :, None]))[0]
        cont = TAURAY if cont is None else cont + TAURAY                                                   # (TAUCIA + TAUDUST) + TAURAY
    P = np.shape(phase_fn)[1]
    taucont = None if cont is None else np.ascontiguousarray(np.transpose(cont.reshape(W, n, L), (1, 0, 2)))
    tausca, phase = np.empty((n, W, L)), np.empty((n, P, W, L))
    for m in range(n):
        s = slice(m * L, (m + 1) * L)
        tausca[m], phase[m] = singlescatt_phase_and_sca(TAUCLSCAT[:, s], TAURAY[:, s], TAUSCAT[:, s], phase_fn)
    return taucont, tausca, phase


class BatchedCKSingleScatterModel:
    """CIRSrad's single-scattering branch (:4251-4336) for n states at once; what `jacobian.jacobian_nemesis_batched` asks of a
    model.

    eng: AnsfmEngine with the k-table uploaded.  state: ContinuousProfileState of T, ln VMR and ln DUST blocks.  ID / ISO,
    igas_map, layering_args, ISPACE, IRAY, PARAH2, cia, dust: as BatchedCKScatterModel takes them; geometry: dict(pointing,
    BOTLAY, ANGLE, EMISS_ANG, IPZEN) of AtmCalc_0 for layering.calc_path, as profile_state.BatchedCKThermalModel takes it.
    phase_fn (NWAVE, NPATH, NDUST + 1): the phase function of every population and, last, of Rayleigh scattering at each
    path's scattering angle (ScatterX.calc_phase / calc_phase_ray, :4269-4271 before the transpose).  SOL_ANG / EMISS_ANG: one
    entry per path; solar (NWAVE); BRDF (NWAVE, NPATH) or None (zeros); TSURF, emissivity (NWAVE; None: 1), xfac (NWAVE) or
    None.  phase_source=(imie, THETA_TAB, tab) with AZI_ANG (one entry per path) instead of phase_fn (pass None): the phase
    function as a resident source of the engine (upload_phase on dust["SWAVE"], uploaded with the aerosol source) and phase_fn
    formed on the device at each path's scattering angle (cirsrad_ck_singlescatt_batch_src).
    More than 7 populations and DUST_RENORMALISATION raise NotImplementedError, as in BatchedCKScatterModel."""

    fused_continuum = True    # False: taucont / tausca / phase of all n * NLAY layers at array level (singlescatt_dense_by_hand)
                              # through cirsrad_ck_singlescatt_batch (same bits)

    def __init__(self, eng, state, RADIUS, ID, ISO, igas_map, phase_fn, SOL_ANG, EMISS_ANG, solar, layering_args=None, geometry=None,
                 ISPACE=0, IRAY=0, PARAH2=None, cia=None, dust=None, BRDF=None, TSURF=-1.0, emissivity=None, xfac=None,
                 DUST_RENORMALISATION=None, phase_source=None, AZI_ANG=None):
        what = "BatchedCKSingleScatterModel: "
        if DUST_RENORMALISATION is not None and DUST_RENORMALISATION is not False:
            raise NotImplementedError(what + "DUST_RENORMALISATION-style rescaling of the aerosol columns is applied by the caller "
                                             "of calc_tau_dust in the reference and is not built here")
        self.dust = None if dust is None else dict(dust)
        has_dust = getattr(state, "has_dust", False)
        DUST = state.DUST if has_dust else (None if self.dust is None else self.dust.get("DUST"))
        if has_dust and self.dust is None:
            raise ValueError(what + "a state with a DUST block needs dust=dict(SWAVE, KEXT, KSCA)")
        if self.dust is not None:
            if DUST is None:
                raise ValueError(what + "no aerosol profiles (a DUST block of the state, or dust['DUST'])")
            DUST = np.asarray(DUST, float).reshape(state.NPRO, -1)
            if max(DUST.shape[1], np.shape(self.dust["KEXT"])[1]) > MAX_POPULATIONS:
                raise NotImplementedError(what + "more than 7 aerosol populations (NumPy sums 8 and more pairwise, the kernels sum "
                                                 "in order)")
            if DUST.shape[1] != np.shape(self.dust["KEXT"])[1] or np.shape(self.dust["KSCA"]) != np.shape(self.dust["KEXT"]):
                raise ValueError(what + "KEXT / KSCA (NWAVE_scatter, NDUST) and DUST (NPRO, NDUST) disagree")
        self.DUST = DUST
        self.ISPACE, self.IRAY, self.TSURF = int(ISPACE), int(IRAY), float(TSURF)
        if self.dust is None and self.IRAY == 0:
            raise ValueError(what + "neither aerosols nor Rayleigh scattering: no scattering opacity")
        self.eng, self.state = eng, state
        self.RADIUS = float(RADIUS)
        self.ID = np.asarray(ID); self.ISO = np.asarray(ISO)
        self.igas_map = np.asarray(igas_map, dtype=np.int64)
        la = dict(NLAY=20, LAYTYP=layering.EQUAL_LOG_PRESSURE, LAYINT=1, LAYHT=0.0, LAYANG=0.0, NINT=101)
        la.update(layering_args or {})
        self.lay = la
        ge = dict(pointing=layering.NADIR, BOTLAY=0, ANGLE=0.0, EMISS_ANG=0.0, IPZEN=layering.IPZEN_BOTTOM)
        ge.update(geometry or {})
        self.geo = ge
        self.cia = None if cia is None else dict(cia)
        self.PARAH2 = PARAH2
        self.SOL_ANG, self.EMISS_ANG = (np.atleast_1d(np.asarray(a, float)) for a in (SOL_ANG, EMISS_ANG))
        dims, _ = eng.ktable_info()
        self.W = int(dims[0])
        self.BASEH, self.BASEP = layering.layer_split(self.RADIUS, state.H, state.P, LAYANG=la["LAYANG"], LAYHT=la["LAYHT"],
                                                      NLAY=la["NLAY"], LAYTYP=la["LAYTYP"])
        self.NPATH = self._path(np.ones_like(self.BASEH), np.ones_like(self.BASEH)).NPATH
        ND = 0 if self.DUST is None else self.DUST.shape[1]
        self.phase_fn = None if phase_fn is None else np.ascontiguousarray(phase_fn, dtype=float)
        self.phase_source = _phase_source(what, phase_source, self.phase_fn, self.dust)
        self.alpha_deg = None
        if self.phase_source is not None:
            if AZI_ANG is None or np.size(AZI_ANG) != self.NPATH or self.phase_source[2].shape[2] != ND:
                raise ValueError(what + "phase_source needs AZI_ANG, one entry per path, and one phase function per population")
            self.alpha_deg = eng.scattering_angle_deg(self.SOL_ANG, self.EMISS_ANG, AZI_ANG)
        elif self.phase_fn is None:
            raise ValueError(what + "phase_fn (NWAVE, NPATH, NDUST + 1) or phase_source is needed")
        elif self.phase_fn.shape != (self.W, self.NPATH, ND + 1):
            raise ValueError(what + "phase_fn must be (NWAVE, NPATH, NDUST + 1) = %s, got %s" % ((self.W, self.NPATH, ND + 1), self.phase_fn.shape))
        if not (self.SOL_ANG.size == self.EMISS_ANG.size == self.NPATH):
            raise ValueError(what + "SOL_ANG and EMISS_ANG list one entry per path")
        self.solar = np.ascontiguousarray(solar, dtype=float)
        self.emissivity = np.ones(self.W) if emissivity is None else np.ascontiguousarray(emissivity, dtype=float)
        self.BRDF = np.zeros((self.W, self.NPATH)) if BRDF is None else np.ascontiguousarray(BRDF, dtype=float).reshape(self.W, self.NPATH)
        self.xfac = None if xfac is None else np.ascontiguousarray(xfac, dtype=float)
        self._sources_on = False
        self.last_rows = (0, 0)       # opacity rows computed / (state, layer) pairs, last spectra_batch
        self.last_shared = False      # the states started their paths from the first state's records, last spectra_batch

    def _path(self, DELH, TEMP):
        ge = self.geo
        return layering.calc_path(self.RADIUS, self.BASEH, DELH, TEMP, float(self.state.H[-1]), pointing=ge["pointing"],
                                  BOTLAY=ge["BOTLAY"], ANGLE=ge["ANGLE"], EMISS_ANG=ge["EMISS_ANG"], IPZEN=ge["IPZEN"])

    # ---- what jacobian_nemesis_batched asks of a model -------------------------------------------------------------
    def ny(self):
        """length of a measurement vector of this model (its wavenumbers x paths)"""
        return self.W * self.NPATH

    def torch_device(self):
        import torch
        return torch.device("cuda", self.eng.device)

    # ---- host part: the profiles, layers and paths of n states ----------------------------------------------------
    def layers(self, X):
        """X (n, NX) -> dict of per-state layer arrays (Layer_0 attributes after calc_layering), the aerosol columns CONT of
        every state's own aerosol profiles among them, `amount` (n, NGAS, NLAY) of the table's gases, VMRLAY and the ray path."""
        st, la = self.state, self.lay
        prof = st.profiles(X)
        T, VMR = prof[0], prof[1]
        n = T.shape[0]
        DUST = prof[2] if len(prof) > 2 else (None if self.DUST is None else np.repeat(self.DUST[None], n, 0))
        H = np.repeat(st.H[None], n, 0); P = np.repeat(st.P[None], n, 0)
        PARAH2 = (self.PARAH2 if self.PARAH2 is None or np.ndim(self.PARAH2) != 1
                  else np.repeat(np.asarray(self.PARAH2, float)[None], n, 0))
        out = self.eng.layer_average(self.RADIUS, H, P, T, self.ID, VMR, DUST, PARAH2, self.BASEH, self.BASEP,
                                     LAYANG=la["LAYANG"], LAYINT=la["LAYINT"], LAYHT=la["LAYHT"], NINT=la["NINT"])
        names = ("HEIGHT", "PRESS", "TEMP", "TOTAM", "AMOUNT", "PP", "CONT", "FRAC", "DELH", "BASET", "LAYSF")
        lay = dict(zip(names, out))
        lay["path"] = self._path(lay["DELH"][0], lay["TEMP"])
        lay["amount"] = np.ascontiguousarray(np.transpose(lay["AMOUNT"][:, :, self.igas_map], (0, 2, 1))) * SQ_CM_TO_SQ_METER
        lay["VMRLAY"] = lay["PP"] / lay["PRESS"][:, :, None]
        return lay

    def upload_sources(self):
        """Make `cia` / `dust` resident sources of the engine, on the grid of the table it holds now."""
        eng = self.eng
        if self.cia is not None:
            c = self.cia
            eng.upload_cia(self.ISPACE, None, c["CIA_WAVEN"], c["CIA_TEMP"], c["CIA_FRAC"], c["NPARA"], c["K_CIA"], c["IPAIRG1"],
                           c["IPAIRG2"], c["INORMALT"], c["INORMAL"], c["INORMALD"], self.ID, self.ISO, k_co2=c.get("k_co2"),
                           k_n2n2=c.get("k_n2n2"), k_n2h2=c.get("k_n2h2"))
        if self.dust is not None:
            eng.upload_dust(self.dust["SWAVE"], self.dust["KEXT"], self.dust["KSCA"])
        if self.phase_source is not None:
            eng.upload_phase(self.phase_source[0], self.dust["SWAVE"], self.phase_source[1], self.phase_source[2])
        self._sources_on = True

    # ---- device part ----------------------------------------------------------------------------------------------
    def spectra_batch(self, X, device=None):
        """Spectra of the n states X (n, NX): torch tensor (n, NY), NY = NWAVE * NPATH (path fastest like SPECOUT), on the
        engine's device."""
        import torch
        eng = self.eng
        dev = torch.device("cuda", eng.device) if device is None else device
        lay = self.layers(X)
        n, L = lay["PRESS"].shape
        path = lay["path"]
        cia, dust = self.cia is not None, self.dust is not None
        rt = (path.NLAYIN, path.LAYINC, np.repeat(path.SCALE[None], n, 0), path.EMTEMP, np.full(n, self.TSURF), self.emissivity,
              self.BRDF, self.solar, self.SOL_ANG, self.EMISS_ANG)
        src = self.phase_source
        if src is not None and not self.fused_continuum:
            raise NotImplementedError("BatchedCKSingleScatterModel: phase_source needs the fused continuum")
        if self.fused_continuum:
            if not self._sources_on:
                self.upload_sources()
            f4 = eng.rayleigh_f4(self.ID, self.ISO, lay["VMRLAY"]) if self.IRAY == 4 else None
            entry = eng.cirsrad_ck_singlescatt_batch_cont if src is None else eng.cirsrad_ck_singlescatt_batch_src
            out = entry(self.ISPACE, lay["PRESS"], lay["TEMP"], lay["amount"],
                        lay["VMRLAY"] if cia else None, lay["FRAC"] if cia else None, lay["TOTAM"],
                        lay["DELH"] if cia else None, lay["CONT"] if dust else None, self.IRAY, f4,
                        self.phase_fn if src is None else self.alpha_deg, *rt, xfac=self.xfac)
        else:
            taucont, tausca, phase = singlescatt_dense_by_hand(eng, self.ISPACE, self.IRAY, self.ID, self.ISO, self.cia, self.dust,
                                                               lay, self.phase_fn)
            out = eng.cirsrad_ck_singlescatt_batch(self.ISPACE, lay["PRESS"], lay["TEMP"], lay["amount"], taucont, tausca, phase,
                                                   *rt, xfac=self.xfac)
        self.last_rows = eng.last_layer_rows()
        self.last_shared = eng.last_rt_shared()
        return torch.as_tensor(out.reshape(n, -1), dtype=torch.float64, device=dev)
