"""Runtime line-by-line (ILBL = LINE_BY_LINE_RUNTIME) as the opacity source of CIRSrad: the host side.

`LineSource` holds what stays fixed over a retrieval -- per gas and isotopologue the lines, the pseudo-continuum bins and
their parameters, after the reference's host-side selections -- in the form `AnsfmEngine.upload_line_source` takes.
`LineSource.from_spectroscopy` builds it from a Spectroscopy object that carries LINE_DATA / LINE_DATA_PARAMS.

`pack_line_state` turns the layers of one or more states into the distinct k-rows of `ansfm_lblrt_set_state`: the
cross-section of gas s in a layer depends on (p, T, the mix fractions of gas s) only, so rows are found per gas by comparing
the bits of those numbers (np.unique on byte views, like `continuum_rows.ContinuumRows`).  The partition-function ratios of a
row follow from its temperature.
"""
import hashlib

import numpy as np

VOIGT, LORENTZ, DOPPLER = 0, 4, 12          # SpectroscopicLineProfileEnum values of the shapes that are built
BUILT_SHAPES = (VOIGT, LORENTZ, DOPPLER)
MAX_NEIGHBOUR_BINS = 8
ATM_TO_PASCAL = 101325.0

_f8 = np.float64


def _a(x, shape=None):
    x = np.ascontiguousarray(x, dtype=_f8)
    if shape is not None and x.shape != shape:
        raise ValueError(f"expected an array of shape {shape}, got {x.shape}")
    return x


class Isotopologue:
    """One isotopologue of a gas.  Lines: bparams (3M, N) = (gamma, n, delta) per broadener, nu / sw / e_lower / stim_ref (N,).
    Bins: pc_bparams (3M, Nb), centers / widths / sw_sum / pc_e_lower (Nb,).  partition_fn: T -> Q(T)."""

    def __init__(self, lineshape_id, abundance, mass, partition_fn, M, *, t_ref=296.0, p_ref=1.0, bparams=None, nu=None, sw=None,
                 e_lower=None, stim_ref=None, s_floor=0.0, wn_calc_window=25.0, wn_approx_window=75.0, include_lines=True,
                 t_cont=296.0, p_cont=1.0, pc_bparams=None, centers=None, widths=None, sw_sum=None, pc_e_lower=None,
                 n_neighbour_bins=3, include_continuum=True):
        self.lineshape_id, self.abundance, self.mass = int(lineshape_id), float(abundance), float(mass)
        self.partition_fn = partition_fn
        self.t_ref, self.p_ref, self.s_floor = float(t_ref), float(p_ref), float(s_floor)
        self.wn_calc_window, self.wn_approx_window = float(wn_calc_window), float(wn_approx_window)
        self.include_lines, self.include_continuum = bool(include_lines), bool(include_continuum)
        self.t_cont, self.p_cont, self.n_neighbour_bins = float(t_cont), float(p_cont), int(n_neighbour_bins)
        self.nu = _a([] if nu is None else nu)
        N = self.N = self.nu.shape[0]
        self.sw, self.e_lower, self.stim_ref = (_a(np.zeros(0) if x is None else x, (N,)) for x in (sw, e_lower, stim_ref))
        self.bparams = _a(np.zeros((3 * M, 0)) if bparams is None else bparams, (3 * M, N))
        self.centers = _a([] if centers is None else centers)
        Nb = self.Nb = self.centers.shape[0]
        self.widths, self.sw_sum, self.pc_e_lower = (_a(np.zeros(0) if x is None else x, (Nb,)) for x in (widths, sw_sum, pc_e_lower))
        self.pc_bparams = _a(np.zeros((3 * M, 0)) if pc_bparams is None else pc_bparams, (3 * M, Nb))

    def unsupported(self):
        """why the device kernels cannot take this isotopologue, or None (the tests of the line and pseudo-continuum entries)"""
        if self.lineshape_id not in BUILT_SHAPES:
            return "a line shape other than Voigt, Lorentz and Doppler"
        if self.include_continuum and self.Nb and np.any(self.sw_sum != 0):
            if self.n_neighbour_bins > MAX_NEIGHBOUR_BINS:
                return "more than 8 neighbour bins"
            if not np.all(self.widths > 0):
                return "pseudo-continuum bin widths that are not positive"
            lo = self.centers - self.widths / 2.0
            if np.any(lo[1:] < lo[:-1]):
                return "pseudo-continuum bins whose lower edges do not ascend"
        return None

    def arrays(self):
        return (self.bparams, self.nu, self.sw, self.e_lower, self.stim_ref, self.pc_bparams, self.centers, self.widths, self.sw_sum,
                self.pc_e_lower)

    def scalars(self):
        return (self.lineshape_id, self.abundance, self.mass, self.t_ref, self.p_ref, self.s_floor, self.wn_calc_window,
                self.wn_approx_window, self.include_lines, self.t_cont, self.p_cont, self.n_neighbour_bins, self.include_continuum)


class LineSource:
    """wn_grid (nw,) ascending wavenumbers; gases: per gas the list of its `Isotopologue`s; M broadeners ("self" + ambient)."""

    def __init__(self, wn_grid, gases, M):
        self.wn_grid = _a(wn_grid)
        self.gases = [list(g) for g in gases]
        self.M = int(M)
        if self.wn_grid.ndim != 1 or self.wn_grid.size == 0 or not self.gases or any(not g for g in self.gases):
            raise ValueError("LineSource: a grid and at least one isotopologue per gas are needed")

    S = property(lambda self: len(self.gases))
    nw = property(lambda self: self.wn_grid.shape[0])
    n_iso = property(lambda self: [len(g) for g in self.gases])

    def unsupported(self):
        if np.any(np.diff(self.wn_grid) < 0):
            return "a wavenumber grid that does not ascend"
        for g in self.gases:
            for iso in g:
                why = iso.unsupported()
                if why:
                    return why
        return None

    def fingerprint(self):
        """content fingerprint of the line data and parameters: the source is uploaded once per fingerprint"""
        h = hashlib.blake2b(digest_size=16)
        h.update(self.wn_grid.tobytes())
        h.update(repr((self.M, self.n_iso)).encode())
        for g in self.gases:
            for iso in g:
                h.update(repr(iso.scalars()).encode())
                for a in iso.arrays():
                    h.update(repr(a.shape).encode())
                    h.update(a.tobytes())
        return h.hexdigest()

    # ---- from the reference's objects -----------------------------------------------------------------------------------
    @classmethod
    def from_spectroscopy(cls, S):
        """The line source of a Spectroscopy object with LINE_DATA (LineData_0 per gas) and LINE_DATA_PARAMS, after the host-side
        selections of LineData_0.add_monochromatic_absorption (LineData_0.py:2282): the inclusive wn_calc_range masks (:882,
        :1376; the range is the grid widened by twice the approximation window, :2328), the zeroed shift rows of
        include_pressure_shift = False (:886-888), the isotopic abundances of :2352-2361, n_neighbour_bins = 3 (:2455)."""
        wave = _a(S.WAVE)
        gases, M = [], None
        for ld, prm in zip(S.LINE_DATA, S.LINE_DATA_PARAMS):
            n_iso = len(ld.line_data)
            if ld.ISO == 0:
                ab = prm.isotopic_abundance
                ab = ld.default_iso_abundances if ab is None else np.atleast_1d(np.asarray(ab, dtype=_f8))
                if len(ab) != n_iso:
                    raise ValueError("there must be an isotopic abundance for each isotopologue in the LineData_0 instance")
            else:
                ab = [1.]
            rng = (np.min(wave) - 2 * prm.wn_approx_window, np.max(wave) + 2 * prm.wn_approx_window)
            isos = []
            for i in range(n_iso):
                ls, pc = ld.line_data[i], ld.continuum_data[i]
                m = len(ls.broadening_molecule_ids)
                if M is not None and m != M:
                    raise ValueError("all LINE_DATA instances must have the same number of ambient gases")
                M = m
                kw = {}
                if ls.has_data:
                    mask = (rng[0] <= ls.NU) & (ls.NU <= rng[1])
                    bp = np.array(ls._data[5:, mask])
                    if not prm.include_pressure_shift:
                        bp[2::3] = bp[2::3] * 0
                    nu, sw, el, sr = (np.array(x) for x in ls._data[:4, mask])
                    kw.update(bparams=bp, nu=nu, sw=sw, e_lower=el, stim_ref=sr)
                if pc is not None and pc.has_data:
                    mask = (rng[0] <= pc.WN_BIN_CENTER) & (pc.WN_BIN_CENTER <= rng[1])
                    c, w, s, e = (np.array(x) for x in pc.WAVE_AND_LINE_DATA[:, mask])
                    kw.update(pc_bparams=np.array(pc.ALL_BROADENING_LSW_PARAMS[:, mask]), centers=c, widths=w, sw_sum=s, pc_e_lower=e,
                              t_cont=pc.t_cont, p_cont=pc.p_cont)
                isos.append(Isotopologue(int(prm.lineshape), ab[i], ls._molecular_mass, ld.partition_fn_data[i], M, t_ref=ls.t_ref,
                                         p_ref=ls.p_ref, s_floor=prm.s_floor, wn_calc_window=prm.wn_calc_window,
                                         wn_approx_window=prm.wn_approx_window, include_lines=prm.include_lines,
                                         include_continuum=prm.include_continuum and pc is not None, n_neighbour_bins=3, **kw))
            gases.append(isos)
        return cls(wave, gases, M)


# ---- the state of a CIRSrad call by distinct k-row -------------------------------------------------------------------------
class LineState:
    """The arguments of `ansfm_lblrt_set_state`: krow (n, S, L) int32 and the R distinct rows, grouped by gas."""

    def __init__(self, krow, row_gas, row_p_atm, row_t, row_mix, row_q_lines, row_q_cont, row_q_lines_dT=None, row_q_cont_dT=None):
        self.krow, self.row_gas = np.ascontiguousarray(krow, dtype=np.int32), np.ascontiguousarray(row_gas, dtype=np.int32)
        self.row_p_atm, self.row_t, self.row_mix = _a(row_p_atm), _a(row_t), _a(row_mix)
        self.row_q_lines, self.row_q_cont = _a(row_q_lines), _a(row_q_cont)
        self.row_q_lines_dT = None if row_q_lines_dT is None else _a(row_q_lines_dT)
        self.row_q_cont_dT = None if row_q_cont_dT is None else _a(row_q_cont_dT)

    n = property(lambda self: self.krow.shape[0])
    S = property(lambda self: self.krow.shape[1])
    L = property(lambda self: self.krow.shape[2])
    R = property(lambda self: self.row_gas.shape[0])
    grad = property(lambda self: self.row_q_lines_dT is not None)


def q_ratios(source, row_gas, row_t):
    """Q(t_ref) / Q(T) of the lines and Q(t_cont) / Q(T) of the bins (LineData_0.py:848, :1374) for every isotopologue of every
    row's gas, one row after the other"""
    ql, qc = [], []
    for s, t in zip(row_gas, row_t):
        for iso in source.gases[int(s)]:
            den = iso.partition_fn(t)
            ql.append(iso.partition_fn(iso.t_ref) / den)
            qc.append(iso.partition_fn(iso.t_cont) / den)
    return np.array(ql, dtype=_f8), np.array(qc, dtype=_f8)


def pack_line_state(source, press_atm, temp, mol_mix_frac, grad=False):
    """press_atm, temp (n, L) or (L,); mol_mix_frac (n, S, M), (S, M) or (M,) -> LineState.  Rows are distinct in the bits of
    (p, T, mix fractions) within a gas and ordered by gas, then by first appearance (state 0's layers first)."""
    p = np.atleast_2d(_a(press_atm))
    t = np.atleast_2d(_a(temp))
    n, L = p.shape
    S, M = source.S, source.M
    mix = _a(mol_mix_frac)
    mix = np.ascontiguousarray(np.broadcast_to(mix, (n, S, M)))
    if t.shape != (n, L):
        raise ValueError("press_atm and temp must have the same shape")
    krow = np.empty((n, S, L), dtype=np.int32)
    gas, rp, rt, rmix = [], [], [], []
    R = 0
    for s in range(S):
        key = np.empty((n, L, 2 + M))
        key[:, :, 0], key[:, :, 1] = p, t
        key[:, :, 2:] = mix[:, s, None, :]
        flat = np.ascontiguousarray(key.reshape(n * L, 2 + M))
        _, first, inv = np.unique(flat.view(np.dtype((np.void, flat.dtype.itemsize * (2 + M)))).ravel(), return_index=True,
                                  return_inverse=True)
        order = np.argsort(first, kind="stable")                      # by first appearance
        rank = np.empty_like(order)
        rank[order] = np.arange(order.size)
        krow[:, s, :] = (R + rank[np.asarray(inv).ravel()]).reshape(n, L)
        rows = flat[first[order]]
        gas.append(np.full(rows.shape[0], s, dtype=np.int32))
        rp.append(rows[:, 0]); rt.append(rows[:, 1]); rmix.append(rows[:, 2:])
        R += rows.shape[0]
    row_gas, row_t = np.concatenate(gas), np.concatenate(rt)
    ql, qc = q_ratios(source, row_gas, row_t)
    qld = qcd = None
    if grad:
        qld, qcd = q_ratios(source, row_gas, row_t + 5.0)             # Spectroscopy_0.py:2021
    return LineState(krow, row_gas, np.concatenate(rp), row_t, np.concatenate(rmix, axis=0), ql, qc, qld, qcd)


def mix_fractions(amb_frac):
    """amb_frac (S, M - 1) -> mol_mix_frac (S, M) = (1 - sum(amb_frac), *amb_frac) as LineData_0.py:2342-2345 forms it"""
    amb = np.atleast_2d(_a(amb_frac))
    return np.array([[1 - sum(row), *row] for row in amb], dtype=_f8)


def ambient_fractions(PP, PRESS, atm_ids, spec_ids):
    """amb_frac (NGAS, 1) of ForwardModel_0.py:3822-3827: one minus the layer-mean mixing ratio of all isotopologues of the gas"""
    ave_vmr = np.mean((np.asarray(PP).T / np.asarray(PRESS)), axis=1)
    atm_ids = np.asarray(atm_ids)
    amb = np.ones((len(spec_ids), 1), dtype=float)
    for igas in range(len(spec_ids)):
        all_iso = np.where(atm_ids == spec_ids[igas])[0]
        amb[igas, 0] = 1.0 - np.sum(ave_vmr[all_iso])
    return amb
