"""AnsfmEngine: one context per GPU around libansfm.so (see include/ansfm.h).

Host-array methods take/return NumPy arrays in the reference's layouts (drop-in for the numba
seams); `*_dev` methods take torch CUDA(HIP) tensors already resident in HBM and run
asynchronously on the engine's stream.  torch is plumbing only (device memory, streams).
"""
import contextlib
import ctypes as C
import os
import numpy as np

from . import _lib

_f8 = np.float64


def _np(a, dtype=_f8):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _is_f32(a):
    return getattr(a, "dtype", None) == np.float32


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(a.data_ptr())  # torch tensor


def _ray_mode(IRAY, variant):
    """ray_mode of include/ansfm.h: IRAY, or 12 for variant='v' (calc_tau_rayleighv)"""
    return 12 if variant == "v" else int(IRAY)


def _fingerprint(a):
    """Identity of a result array handed back to the caller: address, shape and a few sampled values, to recognise
    "the array I returned" when it comes back as the next step's input.  Arrays that have a device twin are handed out
    read-only (flags.writeable = False), so "unmodified" does not rest on the samples: an in-place edit raises, an
    edited copy has another address."""
    flat = a.reshape(-1)
    idx = np.linspace(0, flat.size - 1, num=min(flat.size, 32)).astype(np.int64)
    return (a.ctypes.data, a.shape, a.strides, flat[idx].tobytes())


class _PcArgs:
    """the per-isotopologue arrays of a pseudo-continuum call, contiguous float64 and checked against each other"""

    def __init__(self, L, q_ratio, mol_mix_frac, bparams, centers, widths, sw_sum, e_lower, store, store_x):
        self.q = _np(np.atleast_1d(q_ratio)); self.mmf = _np(mol_mix_frac); self.bp = _np(bparams)
        self.c = _np(centers); self.w = _np(widths); self.sw = _np(sw_sum); self.el = _np(e_lower)
        self.N = N = self.c.shape[0]; self.M = M = self.mmf.shape[0]
        if self.q.shape != (L,):
            raise ValueError("q_ratio must have one value per (T,p) point")
        if self.bp.size != 3 * M * N or any(a.shape != (N,) for a in (self.w, self.sw, self.el)):
            raise ValueError("bin arrays must have shape (N,) and the broadening parameters (3M,N)")
        if store is not None and (store.dtype != np.float64 or not store.flags.c_contiguous or store.size != L * 3 * N):
            raise ValueError("store must be a C-contiguous float64 array of shape (3,N) or (L,3,N)")
        if store_x is not None and (store_x.dtype != np.float64 or not store_x.flags.c_contiguous or store_x.size != L * N):
            raise ValueError("store_x must be a C-contiguous float64 array of shape (N,) or (L,N)")


class AnsfmEngine:
    # `cirsrad_ck_scatter_batch` / `_rows` take phase_of / phasarr_variants (callers tell this engine from older ones and doubles)
    scatter_phase_variants = True

    def __init__(self, device=0):
        self._lib = _lib.load()
        self._ctx = C.c_void_p()
        rc = self._lib.ansfm_create(int(device), C.byref(self._ctx))
        if rc != 0:
            raise _lib.AnsfmError(f"ansfm_create(device={device}) failed ({_lib.ERR_NAMES.get(rc, rc)}): "
                                  "no usable HIP device; there is no CPU fallback")
        self.device = int(device)
        self.dims = None

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.ansfm_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.ansfm_last_error(self._ctx)
            msg = msg.decode() if msg else ""
            exc = ValueError if rc in (1, 4) else (NotImplementedError if rc == 5 else _lib.AnsfmError)
            raise exc(f"{what}: {_lib.ERR_NAMES.get(rc, rc)}: {msg}")

    # ---- stream -------------------------------------------------------------------------------
    def set_stream(self, hip_stream_ptr):
        """Run on the caller's HIP stream.  0 / None = the engine's own (non-blocking) stream: a null handle cannot name the
        legacy default stream through the C-ABI, so code that shares device buffers with another runtime on ITS default
        stream must order the two itself (see `stream_ptr`, `BatchedCKThermalModel.spectra_batch`)."""
        self._check(self._lib.ansfm_set_stream(self._ctx, C.c_void_p(hip_stream_ptr or 0)), "set_stream")
        self._stream_ptr = int(hip_stream_ptr or 0)

    def _order_after_torch(self, t):
        """A torch CUDA tensor handed to a device entry point: unless torch's current stream IS the engine's, wait for what
        torch has queued (its kernels may still be writing the tensor)."""
        try:
            import torch
            cur = torch.cuda.current_stream(t.device)
            if cur.cuda_stream == 0 or cur.cuda_stream != self.stream_ptr:
                cur.synchronize()
        except ImportError:
            pass

    @property
    def stream_ptr(self):
        """handle of the stream the engine was given, 0 while it runs on its own"""
        return getattr(self, "_stream_ptr", 0)

    def synchronize(self):
        self._check(self._lib.ansfm_synchronize(self._ctx), "synchronize")

    def set_gradient_gases(self, gases=None, temperature=True):
        """Spectroscopic gases (indices into the uploaded table) whose amount gradients `cirsradg_ck_*` computes; None = all
        (the reference's behaviour).  The others' parameters come back without their gas part.  temperature=False also
        leaves out the k-table part of the temperature gradient (a state vector without temperature elements).  Sticky."""
        if gases is not None:
            bad = [int(g) for g in gases if not 0 <= int(g) < 31]
            if bad:
                raise ValueError("set_gradient_gases: gas indices must lie in [0, 31) (bit 31 is the temperature slot): %s" % bad)
        mask = 0xFFFFFFFF if gases is None else sum(1 << int(g) for g in set(int(g) for g in gases))
        mask = (mask | 0x80000000) if temperature else (mask & 0x7FFFFFFF)
        self._check(self._lib.ansfm_set_gradient_gases(self._ctx, C.c_uint(mask & 0xFFFFFFFF)), "set_gradient_gases")

    def set_f32_semantics(self, grid_f32, delg_f32):
        """Reproduce NumPy's float32 arithmetic when Spectroscopy_0.PRESS/TEMP (grid) / DELG are
        float32 arrays, as they are after read_tables on .kta files (see include/ansfm.h)."""
        self.grid_f32, self.delg_f32 = bool(grid_f32), bool(delg_f32)
        self._check(self._lib.ansfm_set_f32_semantics(self._ctx, int(self.grid_f32), int(self.delg_f32)),
                    "set_f32_semantics")

    # ---- k-table ------------------------------------------------------------------------------
    def upload_ktable(self, K, PRESS, TEMP, WAVE, DELG):
        """K (W,G,NP,NT,S) float64: NumPy array (host) or torch CUDA tensor (device).
        float32 PRESS/TEMP/DELG arrays switch on the matching float32 semantics."""
        self.set_f32_semantics(_is_f32(PRESS) or _is_f32(TEMP), _is_f32(DELG))
        PRESS = _np(PRESS); TEMP = _np(TEMP); WAVE = _np(WAVE); DELG = _np(DELG)
        W, G, NP, NT, S = (int(x) for x in K.shape)
        assert PRESS.shape == (NP,) and TEMP.shape == (NT,) and WAVE.shape == (W,) and DELG.shape == (G,)
        if isinstance(K, np.ndarray):
            K = _np(K)
            rc = self._lib.ansfm_upload_ktable(self._ctx, W, G, NP, NT, S, _ptr(K), _ptr(PRESS), _ptr(TEMP),
                                               _ptr(WAVE), _ptr(DELG))
        else:
            assert K.is_contiguous() and K.dtype.is_floating_point and K.element_size() == 8
            self._order_after_torch(K)
            rc = self._lib.ansfm_upload_ktable_dev(self._ctx, W, G, NP, NT, S, _ptr(K), _ptr(PRESS), _ptr(TEMP),
                                                   _ptr(WAVE), _ptr(DELG))
        self._check(rc, "upload_ktable")
        self.dims = (W, G, NP, NT, S)
        self.WAVE, self.DELG = WAVE, DELG

    def upload_ktable_files(self, paths, wavemin=0.0, wavemax=1.0e10):
        """Spectroscopy_0.read_tables (:1448) for binary .kta tables, straight from the files into HBM (the float64 K
        array is never built on the host).  Returns WAVE, PRESS, TEMP, DELG of the uploaded table."""
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        rc = self._lib.ansfm_upload_ktable_files(self._ctx, len(paths), arr, float(wavemin), float(wavemax))
        self._check(rc, "upload_ktable_files")
        self.dims, _ = self.ktable_info()
        self.grid_f32 = True
        W, G, NP, NT, S = self.dims
        WAVE, PRESS, TEMP, DELG = np.empty(W), np.empty(NP), np.empty(NT), np.empty(G)
        self._check(self._lib.ansfm_ktable_grids(self._ctx, _ptr(WAVE), _ptr(PRESS), _ptr(TEMP), _ptr(DELG)), "ktable_grids")
        return WAVE, PRESS.astype(np.float32), TEMP.astype(np.float32), DELG.astype(np.float32)

    def upload_lbltable_files(self, paths, wavemin=0.0, wavemax=1.0e10):
        """Spectroscopy_0.read_tables (:1448) for binary .lta LBL tables (ILBL = 2), straight from the files into HBM
        (read_lbltable's Python loop over (wavenumber, pressure) never runs).  Returns WAVE, PRESS, TEMP."""
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        rc = self._lib.ansfm_upload_lbltable_files(self._ctx, len(paths), arr, float(wavemin), float(wavemax))
        self._check(rc, "upload_lbltable_files")
        self.dims, _ = self.ktable_info()
        self.grid_f32 = True
        W, G, NP, NT, S = self.dims
        per_level = _lib.read_lbltable_header(paths[-1])[4] < 0          # NT < 0 in the file: TEMP comes back (NP, |NT|)
        WAVE, PRESS, TEMP, DELG = np.empty(W), np.empty(NP), np.empty((NP, NT) if per_level else NT), np.empty(G)
        self._check(self._lib.ansfm_ktable_grids(self._ctx, _ptr(WAVE), _ptr(PRESS), _ptr(TEMP), _ptr(DELG)), "ktable_grids")
        self.WAVE, self.DELG = WAVE, np.array([1.0])
        return WAVE, PRESS.astype(np.float32), TEMP.astype(np.float32)

    def upload_lbltable(self, K, PRESS, TEMP, WAVE):
        """LBL table (ILBL = 2): K (W,NP,|NT|,S) float64 host array; TEMP (|NT|,) or (NP,|NT|) (NT < 0 form)."""
        self.set_f32_semantics(_is_f32(PRESS) or _is_f32(TEMP), False)
        K = _np(K); PRESS = _np(PRESS); TEMP = _np(TEMP); WAVE = _np(WAVE)
        W, NP, NT, S = (int(x) for x in K.shape)
        temp2d = int(TEMP.ndim == 2)
        assert PRESS.shape == (NP,) and WAVE.shape == (W,) and TEMP.shape == ((NP, NT) if temp2d else (NT,))
        self._check(self._lib.ansfm_upload_lbltable(self._ctx, W, NP, NT, S, _ptr(K), _ptr(PRESS), _ptr(TEMP), temp2d,
                                                    _ptr(WAVE)), "upload_lbltable")
        self.dims = (W, 1, NP, NT, S)
        self.WAVE, self.DELG = WAVE, np.array([1.0])

    def calc_klbl(self, press, temp, grad=False):
        press = _np(press); temp = _np(temp)
        W, _, NP, NT, S = self.dims
        L = press.shape[0]
        k = np.empty((W, L, S)); dk = np.empty((W, L, S)) if grad else None
        self._check(self._lib.ansfm_calc_klbl(self._ctx, L, _ptr(press), _ptr(temp), _ptr(k), _ptr(dk)), "calc_klbl")
        return (k, dk) if grad else k

    # ---- runtime line-by-line (ILBL = 1): the line source resident in the context ---------------------------------------
    def upload_line_source(self, source):
        """`line_source.LineSource` -> HBM (ansfm_lblrt_begin / add_isotopologue / commit): lines sorted and uploaded once.
        The engine then answers like an LBL table with G = 1 and W = nw, its gas opacities coming from the lines; every CIRSrad
        call needs a state first (`set_line_state`).  Uploading a table leaves the mode."""
        g = source.wn_grid
        self._check(self._lib.ansfm_lblrt_begin(self._ctx, source.nw, _ptr(g), source.S, source.M), "lblrt_begin")
        for s, isos in enumerate(source.gases):
            for iso in isos:
                rc = self._lib.ansfm_lblrt_add_isotopologue(
                    self._ctx, s, iso.lineshape_id, iso.abundance, iso.mass, int(iso.include_lines), iso.N, iso.t_ref, iso.p_ref,
                    _ptr(iso.bparams), _ptr(iso.nu), _ptr(iso.sw), _ptr(iso.e_lower), _ptr(iso.stim_ref), iso.s_floor,
                    iso.wn_calc_window, iso.wn_approx_window, int(iso.include_continuum), iso.Nb, iso.t_cont, iso.p_cont,
                    _ptr(iso.pc_bparams), _ptr(iso.centers), _ptr(iso.widths), _ptr(iso.sw_sum), _ptr(iso.pc_e_lower),
                    iso.n_neighbour_bins)
                self._check(rc, "lblrt_add_isotopologue")
        self._check(self._lib.ansfm_lblrt_commit(self._ctx), "lblrt_commit")
        self.dims = (source.nw, 1, 2, 2, source.S)
        self.WAVE, self.DELG = g, np.array([1.0])
        self._line_source = source

    def set_line_state(self, state):
        """`line_source.LineState` (see `line_source.pack_line_state`) -> ansfm_lblrt_set_state: the distinct k-rows are computed
        now and stand for the CIRSrad calls that follow, whose (n_models, L) must be the state's."""
        st = state
        rc = self._lib.ansfm_lblrt_set_state(self._ctx, st.n, st.L, st.R, _ptr(st.krow), _ptr(st.row_gas), _ptr(st.row_p_atm),
                                             _ptr(st.row_t), _ptr(st.row_mix), _ptr(st.row_q_lines), _ptr(st.row_q_cont),
                                             _ptr(st.row_q_lines_dT), _ptr(st.row_q_cont_dT))
        self._check(rc, "lblrt_set_state")

    def set_line_scratch_bytes(self, nbytes):
        """byte budget of the per-(row, line) constants: the rows of a state run in chunks that fit it (no bit depends on it)"""
        self._check(self._lib.ansfm_lblrt_set_scratch_bytes(self._ctx, int(nbytes)), "lblrt_set_scratch_bytes")

    def last_line_rows(self):
        """(rows, (T, p) points, chunks) of the last k-row computation"""
        r, p, c = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.ansfm_lblrt_last(self._ctx, C.byref(r), C.byref(p), C.byref(c)), "lblrt_last")
        return r.value, p.value, c.value

    def calc_klbl_online(self, press, temp, amb_frac, grad=False):
        """Spectroscopy_0.calc_klbl_online (:2046) / calc_klblg_online (:1922) on the uploaded line source: press (atm), temp
        (L,); amb_frac (S, M - 1) or (M - 1,) -> k (nw, L, S) [, dkdT].  Both run calc_klblg_online's summation order."""
        from . import line_source as lsrc
        src = self._line_source
        press = _np(press); temp = _np(temp)
        L = press.shape[0]
        amb = _np(amb_frac)
        mix = lsrc.mix_fractions(np.broadcast_to(amb, (src.S, src.M - 1)))
        def q(t):        # [isotopologues of gas 0, of gas 1, ...][L]
            ql, qc = zip(*(lsrc.q_ratios(src, np.full(L, s), t) for s in range(src.S)))
            return [np.ascontiguousarray(np.concatenate([a.reshape(L, -1).T for a in x], axis=0)) for x in (ql, qc)]
        ql, qc = q(temp)
        k = np.empty((src.nw, L, src.S))
        if grad:
            qld, qcd = q(temp + 5.0)
            dk = np.empty_like(k)
            rc = self._lib.ansfm_calc_klblg_online(self._ctx, L, _ptr(press), _ptr(temp), _ptr(mix), _ptr(ql), _ptr(qc), _ptr(qld),
                                                   _ptr(qcd), _ptr(k), _ptr(dk))
            self._check(rc, "calc_klblg_online")
            return k, dk
        self._check(self._lib.ansfm_calc_klbl_online(self._ctx, L, _ptr(press), _ptr(temp), _ptr(mix), _ptr(ql), _ptr(qc), _ptr(k)),
                    "calc_klbl_online")
        return k

    def ktable_info(self):
        dims = (C.c_int64 * 5)()
        mono = C.c_int()
        self._check(self._lib.ansfm_ktable_info(self._ctx, dims, C.byref(mono)), "ktable_info")
        return tuple(int(d) for d in dims), bool(mono.value)

    def ktable_has_boxed(self):
        """True when some entry of the uploaded table is <= 0 or NaN (the merge then keeps its box tests)."""
        b = C.c_int()
        self._check(self._lib.ansfm_ktable_has_boxed(self._ctx, C.byref(b)), "ktable_has_boxed")
        return bool(b.value)

    def last_merge_launch(self):
        """(waves per block, trim bits) of the last forward merge launch: bits 1 weight table, 2 key repack,
        8 list pass that ends at the insertion point, 16 per-lane row operand, 32 a wave's lanes grouped over rows
        (at either width, see last_merge_group_width; clear with ANSFM_MERGE_LANES=wavenumbers and for a launch of 2^24 (model, layer) rows or more, which keeps 64
        wavenumbers of one row per wave), 64 row-major merges are walked without the head list (kernels with bit 1; clear with
        ANSFM_MERGE_ROWMAJOR=0) (4: retired, never set)."""
        w, t = C.c_int(), C.c_int()
        self._check(self._lib.ansfm_last_merge_launch(self._ctx, C.byref(w), C.byref(t)), "last_merge_launch")
        return int(w.value), int(t.value)

    def last_merge_group_width(self):
        """Wavenumbers per wave of the last forward merge launch where its lanes were grouped over rows (bit 32 of
        last_merge_launch's trims): 1 (64 rows of one wavenumber, the library's choice) or 2 (ANSFM_MERGE_LANES=pairs);
        0 where a wave held 64 wavenumbers of one row."""
        w = C.c_int()
        self._check(self._lib.ansfm_last_merge_group_width(self._ctx, C.byref(w)), "last_merge_group_width")
        return int(w.value)

    def ktable_gfast(self):
        """(present, bytes) of the g-fastest copy of the uploaded k-table (built at the upload unless ANSFM_TABLE_GFAST=0, not
        for G = 1 or an LBL table): (False, 0) without it."""
        p, b = C.c_int(), C.c_int64()
        self._check(self._lib.ansfm_ktable_gfast(self._ctx, C.byref(p), C.byref(b)), "ktable_gfast")
        return bool(p.value), int(b.value)

    def last_merge_table_layout(self):
        """True when the last forward merge launch read the table from its g-fastest copy (ktable_gfast; ANSFM_TABLE_LAYOUT=wave
        at the call keeps the wave-fastest reads)."""
        g = C.c_int()
        self._check(self._lib.ansfm_last_merge_table_layout(self._ctx, C.byref(g)), "last_merge_table_layout")
        return bool(g.value)

    def last_merge_rowmajor(self):
        """(merges walked row by row, merges) of the last forward merge launch, counted per wave: a wave whose lanes' G x G sums
        all sort row by row walks that merge without the head list (bit 64 of last_merge_launch's trims; off with
        ANSFM_MERGE_ROWMAJOR=0).  (0, 0) for a kernel without the weight table, which does not count."""
        m, t = C.c_int64(), C.c_int64()
        self._check(self._lib.ansfm_last_merge_rowmajor(self._ctx, C.byref(m), C.byref(t)), "last_merge_rowmajor")
        return int(m.value), int(t.value)

    def last_merge_suffix(self):
        """(rows walked behind a list phase, rows of the merges not walked whole) of the last forward merge launch, counted per
        wave: a merge whose rows i0 .. G-1 sort row by row above everything in the rows below runs the head list for those
        rows only and walks the rest (at least two rows; same bits; off with ANSFM_MERGE_SUFFIX=0 and with the walk).
        (0, 0) for a kernel without the weight table."""
        r, t = C.c_int64(), C.c_int64()
        self._check(self._lib.ansfm_last_merge_suffix(self._ctx, C.byref(r), C.byref(t)), "last_merge_suffix")
        return int(r.value), int(t.value)

    def last_merge_static(self):
        """(merges walked on the static schedule, valid) of the last forward merge launch, counted per wave as
        last_merge_rowmajor counts: a merge that is walked whole closes its bins where del_g alone says, so a launch with
        float32 weights and G > 10 takes the crossings from a schedule formed on the host (same bits; off with
        ANSFM_MERGE_STATIC=0 and with the walk).  valid: the launch carried a valid schedule."""
        m, v = C.c_int64(), C.c_int()
        self._check(self._lib.ansfm_last_merge_static(self._ctx, C.byref(m), C.byref(v)), "last_merge_static")
        return int(m.value), bool(v.value)

    def last_merge_order(self):
        """(applied, non-zero bytes) of the last forward merge launch: applied when it handed the wavenumbers of a block out in
        the order of the pattern bytes that the launch before wrote (the same table upload or the seam, W, rows, S and G; the
        library's own launch at group width 1 with the walk on and G > 10; off with ANSFM_MERGE_ORDER=0), and how many of the bytes it
        read were not 0.  (False, 0) for every other launch."""
        a, n = C.c_int(), C.c_int64()
        self._check(self._lib.ansfm_last_merge_order(self._ctx, C.byref(a), C.byref(n)), "last_merge_order")
        return bool(a.value), int(n.value)

    # ---- array-level seams --------------------------------------------------------------------
    def calc_k(self, press, temp, grad=False):
        press = _np(press); temp = _np(temp)
        W, G, NP, NT, S = self.dims
        L = press.shape[0]
        k = np.empty((W, G, L, S)); dk = np.empty((W, G, L, S)) if grad else None
        self._check(self._lib.ansfm_calc_k(self._ctx, L, _ptr(press), _ptr(temp), _ptr(k), _ptr(dk)), "calc_k")
        return (k, dk) if grad else k

    def k_overlap(self, del_g, k_w_g_l_gas, amount_layer):
        self.set_f32_semantics(getattr(self, "grid_f32", False), _is_f32(del_g))
        del_g = _np(del_g); k = _np(k_w_g_l_gas); am = _np(amount_layer)
        W, G, L, S = k.shape
        if am.shape != (S, L):
            raise ValueError("amount_layer must be (NGAS, NLAYER)")
        tau = np.empty((W, G, L))
        self._check(self._lib.ansfm_k_overlap(self._ctx, W, G, L, S, _ptr(del_g), _ptr(k), _ptr(am), _ptr(tau)),
                    "k_overlap")
        return tau

    def k_overlapg(self, del_g, k_w_g_l_gas, dkdT_w_g_l_gas, amount_layer):
        self.set_f32_semantics(getattr(self, "grid_f32", False), _is_f32(del_g))
        del_g = _np(del_g); k = _np(k_w_g_l_gas); dkdT = _np(dkdT_w_g_l_gas); am = _np(amount_layer)
        W, G, L, S = k.shape
        if am.shape != (S, L) or dkdT.shape != k.shape:
            raise ValueError("shapes: k, dkdT (NWAVE,NG,NLAYER,NGAS); amount (NGAS,NLAYER)")
        tau = np.empty((W, G, L)); dk = np.empty((W, G, L, S + 1))
        self._check(self._lib.ansfm_k_overlapg(self._ctx, W, G, L, S, _ptr(del_g), _ptr(k), _ptr(dkdT), _ptr(am),
                                               _ptr(tau), _ptr(dk)), "k_overlapg")
        return tau, dk

    def calc_thermal_emission_spectrum(self, ISPACE, WAVE, TAUTOT_PATH, EMITOT_PATH, TEMP, PRESS, TSURF,
                                       EMISSIVITY, SOLFLUX, REFLECTANCE, SOL_ANG, EMISS_ANG):
        WAVE = _np(WAVE); TAU = _np(TAUTOT_PATH); EMI = _np(EMITOT_PATH)
        W, G, Li = TAU.shape
        out = np.empty((W, G))
        rc = self._lib.ansfm_thermal_emission(self._ctx, int(ISPACE), W, G, Li, _ptr(WAVE), _ptr(TAU), _ptr(EMI),
                                              _ptr(_np(TEMP)), _ptr(_np(PRESS)), float(TSURF),
                                              _ptr(_np(EMISSIVITY)), _ptr(_np(SOLFLUX)), _ptr(_np(REFLECTANCE)),
                                              float(SOL_ANG), float(EMISS_ANG), _ptr(out))
        self._check(rc, "thermal_emission")
        return out

    # ---- fused CIRSrad (batch) ----------------------------------------------------------------
    def _layer_args(self, what, lay_press_pa, lay_temp, amount, taucont=None, dtaucon=None, NPAR=None, *, model_axis, dims=None):
        """The layer arrays of a CIRSrad entry as the library takes them -> n, L, single, lp (n, L), lt (n, L), am (n, NGAS, L),
        tc (n, NWAVE, L) or None, dtc (n, NWAVE, NPAR, L) or None, contiguous float64.  model_axis: "optional" -- a leading
        model axis or none (single: there was none, and the results drop it again); "required" -- lay_press_pa (n, L), and
        lay_temp and amount exactly (n, L) and (n, NGAS, L); "none" -- one model, lay_press_pa (L,).  dims: those of the table
        where the entry asks `ktable_info()` for them, else `self.dims`."""
        dims = self.dims if dims is None else dims
        W, S = dims[0], dims[4]
        lp, lt, am = _np(lay_press_pa), _np(lay_temp), _np(amount)
        single = lp.ndim == 1
        if model_axis == "required":
            if lp.ndim != 2:
                raise ValueError(f"{what}: lay_press_pa must be (n_models, NLAY)")
            n, L = lp.shape
            if lt.shape != (n, L):
                raise ValueError(f"{what}: lay_temp must be (n_models, NLAY)")
            if am.shape != (n, S, L):
                raise ValueError(f"{what}: amount must be (n_models, NGAS, NLAY)")
        else:
            if model_axis == "none" and not single:
                raise ValueError(what + ": one model, lay_press_pa (NLAY,)")
            lp = np.atleast_2d(lp); n, L = lp.shape
            lt = lt.reshape(1, L) if model_axis == "none" else np.atleast_2d(lt)
            am = am.reshape(n, S, L)
        tc = None if taucont is None else _np(taucont).reshape(n, W, L)
        dtc = None if dtaucon is None else _np(dtaucon).reshape(n, W, int(NPAR), L)
        return n, L, single, lp, lt, am, tc, dtc

    @staticmethod
    def _path_args(what, NLAYIN, LAYINC, SCALE=None, EMTEMP=None, TSURF=None, n=1, exact=False):
        """The path arrays of a CIRSrad entry -> int32 NLAYIN (P,) and LAYINC (LIMAX, P) (a 1-D LAYINC is one path), LIMAX, P,
        and, where given, SCALE / EMTEMP (n, LIMAX, P) and TSURF (n,).  SCALE / EMTEMP are read as a stack of (LIMAX, P)
        blocks, whatever their shape (`reshape(-1, LIMAX, P)`): one block serves every model, n blocks are the models'.
        exact: only the shapes (LIMAX, P) and (n, LIMAX, P) are taken, so a transposed array is refused, not reread.
        ValueError where NLAYIN is not (P,): the library reads P entries of it."""
        LAYINC = _np(LAYINC, np.int32); NLAYIN = _np(np.atleast_1d(NLAYIN), np.int32)
        if LAYINC.ndim == 1:
            LAYINC = LAYINC[:, None]
        LIMAX, P = LAYINC.shape
        if NLAYIN.shape != (P,):
            raise ValueError(f"{what}: NLAYIN must be (NPATH,)")

        def over(name, a):
            if a is None:
                return None
            a = _np(a)
            if exact and a.shape not in ((LIMAX, P), (n, LIMAX, P)):
                raise ValueError(f"{what}: {name} must be {(n, LIMAX, P)} or {(LIMAX, P)}, got {a.shape}")
            return _np(np.broadcast_to(a.reshape(-1, LIMAX, P), (n, LIMAX, P)))
        TS = None if TSURF is None else _np(np.broadcast_to(np.atleast_1d(_np(TSURF)), (n,)))
        return NLAYIN, LAYINC, LIMAX, P, over("SCALE", SCALE), over("EMTEMP", EMTEMP), TS

    @staticmethod
    def _per_model_tsurf(what, TSURF, n):
        TS = _np(np.atleast_1d(TSURF))
        if TS.shape != (n,):
            raise ValueError(f"{what}: TSURF must be (n_models,)")
        return TS

    def _gradient_result(self, single, spec, dspec, dts=None, device_chain=None):
        """What a `cirsradg_ck_*` entry with a model axis hands back, and the chain to map2pro: device_chain (W, NPAR, LIMAX,
        P) where dSPECOUT stayed on the device (dspec is None); else one model's dSPECOUT has a device twin, so the host array
        goes out read-only and is recognised when it comes back.  The caller cleared the chain before the library call."""
        if device_chain is not None:
            self._chain_dspec = ("device",) + tuple(device_chain)
        elif spec.shape[0] == 1:
            dspec.flags.writeable = False
            self._chain_dspec = _fingerprint(dspec[0])
        out = (spec, dspec) if dts is None else (spec, dspec, dts)
        return tuple(None if a is None else a[0] for a in out) if single else out

    def _fused_gradient_call(self, what, L, dtau_every_gas, gradients_on_device, gshape, args, outs):
        """One body for the fused one-model routes (transit, occultation, limb, disc): args are the library's arguments
        between ctx and the outputs, outs the host outputs before the gradient, gshape (W, NPAR, L) or (W, NPAR, L, Q) the
        gradient's.  Clears the chain, calls with dtau_every_gas armed, and arms ("device", W, NPAR, L, Q) where the gradient
        stayed on the device.  -> (*outs, gradient or None)"""
        grad = None if gradients_on_device else np.empty(gshape)
        with self._shared_gas_gradient(what, dtau_every_gas, L):
            self._chain_dspec = None
            rc = getattr(self._lib, "ansfm_" + what)(self._ctx, *args, *(_ptr(o) for o in outs), _ptr(grad))
        self._check(rc, what)
        if gradients_on_device:
            self._chain_dspec = ("device",) + tuple(gshape) + (() if len(gshape) == 4 else (1,))
        return (*outs, grad)

    def calc_thermal_emission_spectrumg(self, ISPACE, WAVE, TAUTOT_PATH, dTAUTOT_PATH, NVMR, TEMP, PRESS, TSURF, EMISSIVITY):
        """ForwardModel_0.calc_thermal_emission_spectrumg (:6380), same arguments -> SPECOUT (NWAVE, NG),
        dSPECOUT (NWAVE, NG, NPAR, NLAYIN), dTSURF (NWAVE, NG)."""
        TAU = _np(TAUTOT_PATH); dTAU = _np(dTAUTOT_PATH)
        W, G, NPAR, Li = dTAU.shape
        if TAU.shape != (W, G, Li):
            raise ValueError("TAUTOT_PATH must be (NWAVE, NG, NLAYIN) and dTAUTOT_PATH (NWAVE, NG, NPAR, NLAYIN)")
        spec = np.empty((W, G)); dspec = np.empty((W, G, NPAR, Li)); dts = np.empty((W, G))
        rc = self._lib.ansfm_thermal_emission_g(self._ctx, int(ISPACE), W, G, NPAR, Li, _ptr(_np(WAVE)), _ptr(TAU), _ptr(dTAU),
                                                int(NVMR), _ptr(_np(TEMP)), _ptr(_np(PRESS)), float(TSURF), _ptr(_np(EMISSIVITY)),
                                                _ptr(spec), _ptr(dspec), _ptr(dts))
        self._check(rc, "thermal_emission_g")
        return spec, dspec, dts

    def cirsrad_ck_thermal(self, ISPACE, lay_press_pa, lay_temp, amount, taucont, NLAYIN, LAYINC, SCALE, EMTEMP,
                           TSURF, EMISSIVITY=None, SOLFLUX=None, REFLECTANCE=None, SOL_ANG=None, EMISS_ANG=None,
                           xfac=None):
        """Host arrays; leading model axis optional.  Returns SPECOUT (n,W,P) (or (W,P))."""
        what, W = "cirsrad_ck_thermal", self.dims[0]
        n, L, single, lp, lt, am, tc, _ = self._layer_args(what, lay_press_pa, lay_temp, amount, taucont, model_axis="optional")
        NLAYIN, LAYINC, LIMAX, P, SC, ET, TS = self._path_args(what, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, n)
        out = np.empty((n, W, P))
        rc = self._lib.ansfm_cirsrad_ck_thermal(
            self._ctx, int(ISPACE), n, L, _ptr(lp), _ptr(lt), _ptr(am), _ptr(tc), P, LIMAX, _ptr(NLAYIN),
            _ptr(LAYINC), _ptr(SC), _ptr(ET), _ptr(TS), _ptr(_np(EMISSIVITY)), _ptr(_np(SOLFLUX)),
            _ptr(_np(REFLECTANCE)), _ptr(None if SOL_ANG is None else _np(np.atleast_1d(SOL_ANG))),
            _ptr(None if EMISS_ANG is None else _np(np.atleast_1d(EMISS_ANG))), _ptr(_np(xfac)), _ptr(out))
        self._check(rc, what)
        return out[0] if single else out

    def calc_singlescatt_plane_spectrum(self, ISPACE, WAVE, TAUTOT_PATH, TEMP, OMEGA, PHASE, TSURF, EMISSIVITY, BRDF, SOLFLUX,
                                        SOL_ANG, EMISS_ANG):
        """ForwardModel_0.calc_singlescatt_plane_spectrum (:6509), same arguments -> SPECOUT (NWAVE, NG)."""
        TAU = _np(TAUTOT_PATH); W, G, Li = TAU.shape
        out = np.empty((W, G))
        rc = self._lib.ansfm_singlescatt_plane_spectrum(
            self._ctx, int(ISPACE), W, G, Li, _ptr(_np(WAVE)), _ptr(TAU), _ptr(_np(TEMP)), _ptr(_np(OMEGA).reshape(W, G, Li)),
            _ptr(_np(PHASE).reshape(W, Li)), float(TSURF), _ptr(_np(EMISSIVITY)), _ptr(_np(BRDF)), _ptr(_np(SOLFLUX)),
            float(SOL_ANG), float(EMISS_ANG), _ptr(out))
        self._check(rc, "singlescatt_plane_spectrum")
        return out

    def cirsrad_ck_singlescatt(self, ISPACE, lay_press_pa, lay_temp, amount, taucont, tausca, phase, NLAYIN, LAYINC, SCALE, EMTEMP,
                               TSURF, EMISSIVITY, BRDF, SOLFLUX, SOL_ANG, EMISS_ANG, xfac=None):
        """CIRSrad, single-scattering branch (:4251-4336) on the uploaded k-table: taucont / tausca (NWAVE, NLAY), phase
        (NPATH, NWAVE, NLAY), BRDF (NWAVE, NPATH) -> SPECOUT (NWAVE, NPATH)."""
        W, G, NP, NT, S = self.dims
        lp = _np(lay_press_pa); L = lp.shape[0]
        NLAYIN, LAYINC, LIMAX, P, SC, ET, _ = self._path_args("cirsrad_ck_singlescatt", NLAYIN, LAYINC, SCALE, EMTEMP)
        out = np.empty((W, P))
        rc = self._lib.ansfm_cirsrad_ck_singlescatt(
            self._ctx, int(ISPACE), L, _ptr(lp), _ptr(_np(lay_temp)), _ptr(_np(amount).reshape(S, L)),
            _ptr(None if taucont is None else _np(taucont).reshape(W, L)), _ptr(_np(tausca).reshape(W, L)),
            _ptr(_np(phase).reshape(P, W, L)), P, LIMAX, _ptr(NLAYIN), _ptr(LAYINC), _ptr(SC), _ptr(ET), float(TSURF),
            _ptr(_np(EMISSIVITY)), _ptr(_np(BRDF).reshape(W, P)),
            _ptr(_np(SOLFLUX)), _ptr(_np(np.atleast_1d(SOL_ANG))), _ptr(_np(np.atleast_1d(EMISS_ANG))), _ptr(_np(xfac)), _ptr(out))
        self._check(rc, "cirsrad_ck_singlescatt")
        return out

    def cirsrad_ck_singlescatt_batch(self, ISPACE, lay_press_pa, lay_temp, amount, taucont, tausca, phase, NLAYIN, LAYINC, SCALE,
                                     EMTEMP, TSURF, EMISSIVITY, BRDF, SOLFLUX, SOL_ANG, EMISS_ANG, xfac=None):
        """The single-scattering branch of CIRSrad for the n forward models of a numerical Jacobian
        (ansfm_cirsrad_ck_singlescatt_batch): lay_press_pa / lay_temp (n, NLAY), amount (n, NGAS, NLAY), taucont / tausca
        (n, NWAVE, NLAY) (taucont may be None), phase (n, NPATH, NWAVE, NLAY), SCALE / EMTEMP (n, LIMAX, NPATH), TSURF (n,); the
        rest as `cirsrad_ck_singlescatt`, shared by the models -> SPECOUT (n, NWAVE, NPATH).
        Only the distinct (model, layer) gas opacities are computed (`last_layer_rows()`), and every state starts each path
        from the record model 0 left after the last layer the two have in common (`last_rt_shared()`).  The same numbers as n
        `cirsrad_ck_singlescatt` calls, bit for bit."""
        what, W = "cirsrad_ck_singlescatt_batch", self.dims[0]
        n, L, _, lp, lt, am, tc, _ = self._layer_args(what, lay_press_pa, lay_temp, amount, taucont, model_axis="required")
        NLAYIN, LAYINC, LIMAX, P, SC, ET, _ = self._path_args(what, NLAYIN, LAYINC, SCALE, EMTEMP, n=n)
        TS = self._per_model_tsurf(what, TSURF, n)
        out = np.empty((n, W, P))
        rc = self._lib.ansfm_cirsrad_ck_singlescatt_batch(
            self._ctx, int(ISPACE), n, L, _ptr(lp), _ptr(lt), _ptr(am), _ptr(tc), _ptr(_np(tausca).reshape(n, W, L)),
            _ptr(_np(phase).reshape(n, P, W, L)), P, LIMAX, _ptr(NLAYIN), _ptr(LAYINC), _ptr(SC), _ptr(ET), _ptr(TS),
            _ptr(_np(EMISSIVITY)), _ptr(_np(BRDF).reshape(W, P)), _ptr(_np(SOLFLUX)), _ptr(_np(np.atleast_1d(SOL_ANG))),
            _ptr(_np(np.atleast_1d(EMISS_ANG))), _ptr(_np(xfac)), _ptr(out))
        self._check(rc, what)
        return out

    def cirsrad_ck_singlescatt_batch_cont(self, ISPACE, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, phase_fn,
                                          NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, BRDF, SOLFLUX, SOL_ANG, EMISS_ANG,
                                          xfac=None, variant=None):
        """`cirsrad_ck_singlescatt_batch` with taucont, tausca and phase formed inside the call, once per distinct layer, from
        the resident sources (upload_cia, upload_dust) and the Rayleigh parametrisations
        (ansfm_cirsrad_ck_singlescatt_batch_cont): q (n, NLAY, NVMR) = PP / PRESS with FRAC, DELH (n, NLAY) switch CIA on (None:
        off); CONT (n, NLAY, NDUST) switches the aerosols on (None: off; NDUST as uploaded); IRAY 0, 1, 2 or 4 (variant='v':
        calc_tau_rayleighv) with f4 (n, NLAY, 4) for IRAY 4 (`rayleigh_f4`); TOTAM (n, NLAY) for CIA and Rayleigh; phase_fn
        (NWAVE, NPATH, NDUST + 1): the phase function of every population and, last, of Rayleigh scattering at each path's
        scattering angle (ScatterX.calc_phase / calc_phase_ray).  Host arrays; the rest as `cirsrad_ck_singlescatt_batch` ->
        SPECOUT (n, NWAVE, NPATH), bit-identical to that call on the dense arrays of calc_tau_cia / calc_tau_dust /
        calc_tau_rayleigh put together as ForwardModel_0.py:3963-3989 and :4316-4321 do."""
        return self._singlescatt_cont("cirsrad_ck_singlescatt_batch_cont", ISPACE, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH,
                                      CONT, IRAY, f4, phase_fn, None, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, BRDF, SOLFLUX,
                                      SOL_ANG, EMISS_ANG, xfac, variant)

    def cirsrad_ck_singlescatt_batch_src(self, ISPACE, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, alpha_deg,
                                         NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, BRDF, SOLFLUX, SOL_ANG, EMISS_ANG,
                                         xfac=None, variant=None):
        """`cirsrad_ck_singlescatt_batch_cont` with phase_fn formed on the device from the resident phase-function source
        (upload_phase) and the Rayleigh formula (ansfm_cirsrad_ck_singlescatt_batch_src): alpha_deg (NPATH,) is each path's
        scattering angle in degrees, `scattering_angle_deg(SOL_ANG, EMISS_ANG, AZI_ANG)`.  Bit-identical to the `_cont` call with
        phase_fn put together from `phase_from_source(alpha_deg)` and `calc_phase_ray(alpha_deg)`."""
        return self._singlescatt_cont("cirsrad_ck_singlescatt_batch_src", ISPACE, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH,
                                      CONT, IRAY, f4, None, alpha_deg, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, BRDF, SOLFLUX,
                                      SOL_ANG, EMISS_ANG, xfac, variant)

    @staticmethod
    def scattering_angle_deg(SOL_ANG, EMISS_ANG, AZI_ANG):
        """the scattering angle of each path in degrees, by the expression of ForwardModel_0.py:4265-4270"""
        sol_ang, emiss_ang, azi_ang = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (SOL_ANG, EMISS_ANG, AZI_ANG))
        calpha = np.sin(sol_ang / 180. * np.pi) * np.sin(emiss_ang / 180. * np.pi) * np.cos(azi_ang / 180. * np.pi - np.pi) - \
            np.cos(emiss_ang / 180. * np.pi) * np.cos(sol_ang / 180. * np.pi)
        return np.arccos(calpha) / np.pi * 180.

    def _fused_cont_args(self, what, n, L, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, variant, dev=False, ncont=None):
        """The continuum formed inside a call from the resident sources, as every entry that has one takes it: use_cia, lay_q,
        lay_frac, lay_totam, lay_delh, use_dust, lay_cont, ray_mode, f4 of include/ansfm.h for n states of L layers.  q given
        switches CIA on, CONT the aerosols; ray_mode is IRAY, or 12 for variant='v' (calc_tau_rayleighv).  dev: the arrays are
        contiguous float64 torch device tensors, else host arrays.  ncont: the populations CONT must have (None: as many as it
        has).  -> (the nine ctypes arguments, the populations of CONT); ValueError for an array of another shape and for a
        term without its arrays."""
        mode = _ray_mode(IRAY, variant)
        use_cia, use_dust = q is not None, CONT is not None
        if not dev:
            q, FRAC, TOTAM, DELH, CONT, f4 = (_np(a) for a in (q, FRAC, TOTAM, DELH, CONT, f4))
        if ncont is None:
            ncont = CONT.shape[-1] if use_dust else 0
        for name, a, dims, shape in (("q", q, "(n_models, NLAY, NVMR of upload_cia)", (n, L, getattr(self, "cia_nvmr", -1))),
                                     ("FRAC", FRAC, "(n_models, NLAY)", (n, L)), ("TOTAM", TOTAM, "(n_models, NLAY)", (n, L)),
                                     ("DELH", DELH, "(n_models, NLAY)", (n, L)), ("CONT", CONT, "(n_models, NLAY, NDUST)", (n, L, ncont)),
                                     ("f4", f4, "(n_models, NLAY, 4)", (n, L, 4))):
            if a is not None and -1 not in shape and (tuple(a.shape) != shape or (dev and not a.is_contiguous())):
                raise ValueError(f"{what}: {name} must be {'a contiguous tensor ' if dev else ''}{dims} = {shape}, got {tuple(a.shape)}")
        if use_cia and (FRAC is None or DELH is None):
            raise ValueError(f"{what}: CIA (q given) needs FRAC and DELH")
        if (use_cia or mode) and TOTAM is None:
            raise ValueError(f"{what}: CIA and Rayleigh need TOTAM")
        if mode == 4 and f4 is None:
            raise ValueError(f"{what}: IRAY 4 needs f4 (rayleigh_f4)")
        return (int(use_cia), _ptr(q), _ptr(FRAC), _ptr(TOTAM), _ptr(DELH), int(use_dust), _ptr(CONT), mode,
                _ptr(f4) if mode == 4 else None), (ncont if use_dust else 0)

    def _singlescatt_cont(self, what, ISPACE, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, phase_fn, alpha_deg,
                          NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, BRDF, SOLFLUX, SOL_ANG, EMISS_ANG, xfac, variant):
        """the `_cont` entry (phase_fn) or the `_src` entry (alpha_deg)"""
        src = what.endswith("_src")
        dims, _ = self.ktable_info()
        W = dims[0]
        n, L, _, lp, lt, am, _, _ = self._layer_args(what, lay_press_pa, lay_temp, amount, model_axis="required", dims=dims)
        NLAYIN, LAYINC, LIMAX, P, SC, ET, _ = self._path_args(what, NLAYIN, LAYINC, SCALE, EMTEMP, n=n, exact=True)
        TS = self._per_model_tsurf(what, TSURF, n)
        cont, ncont = self._fused_cont_args(what, n, L, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, variant)
        arrs = {}
        for name, a, shape in (("phase_fn", phase_fn, (W, P, ncont + 1)),
                               ("alpha_deg", None if alpha_deg is None else np.atleast_1d(alpha_deg), (P,)),
                               ("BRDF", BRDF, (W, P)), ("EMISSIVITY", EMISSIVITY, (W,)),
                               ("SOLFLUX", SOLFLUX, (W,)), ("xfac", xfac, (W,)), ("SOL_ANG", None if SOL_ANG is None else np.atleast_1d(SOL_ANG), (P,)),
                               ("EMISS_ANG", None if EMISS_ANG is None else np.atleast_1d(EMISS_ANG), (P,))):
            a = arrs[name] = None if a is None else _np(a)
            if a is not None and a.shape != shape:
                raise ValueError(f"{what}: {name} must be {shape}, got {a.shape}")
        if arrs["alpha_deg" if src else "phase_fn"] is None:
            raise ValueError(f"{what}: " + ("alpha_deg (NPATH,)" if src else "phase_fn (NWAVE, NPATH, NDUST + 1)") + " is needed")
        out = np.empty((n, W, P))
        rc = getattr(self._lib, "ansfm_" + what)(
            self._ctx, int(ISPACE), n, L, _ptr(lp), _ptr(lt), _ptr(am), *cont, ncont,
            _ptr(arrs["alpha_deg" if src else "phase_fn"]), P, LIMAX, _ptr(NLAYIN), _ptr(LAYINC), _ptr(SC), _ptr(ET),
            _ptr(TS), _ptr(arrs["EMISSIVITY"]), _ptr(arrs["BRDF"]), _ptr(arrs["SOLFLUX"]), _ptr(arrs["SOL_ANG"]), _ptr(arrs["EMISS_ANG"]),
            _ptr(arrs["xfac"]), _ptr(out))
        self._check(rc, what)
        return out

    def cirsrad_ck_transmission(self, lay_press_pa, lay_temp, amount, taucont, NLAYIN, LAYINC, SCALE, xfac=None):
        """CIRSrad, pure-transmission branch (calculate_transmission_spectrum :4110): SPECOUT (n, W, P) (or (W, P)) =
        xfac * sum_g DELG exp(-sum over the path's layers of TAUTOT_LAYINC)."""
        what, W = "cirsrad_ck_transmission", self.dims[0]
        n, L, single, lp, lt, am, tc, _ = self._layer_args(what, lay_press_pa, lay_temp, amount, taucont, model_axis="optional")
        NLAYIN, LAYINC, LIMAX, P, SC, _, _ = self._path_args(what, NLAYIN, LAYINC, SCALE, n=n)
        out = np.empty((n, W, P))
        rc = self._lib.ansfm_cirsrad_ck_transmission(self._ctx, n, L, _ptr(lp), _ptr(lt), _ptr(am), _ptr(tc), P, LIMAX, _ptr(NLAYIN),
                                                     _ptr(LAYINC), _ptr(SC), _ptr(_np(xfac)), _ptr(out))
        self._check(rc, what)
        return out[0] if single else out

    def cirsradg_ck_transmission(self, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map, NLAYIN,
                                 LAYINC, SCALE, xfac=None):
        """CIRSrad(return_grad=True), pure-transmission branch (:4110-4131, :4504-4507): SPECOUT (n, W, P) and
        dSPECOUT (n, W, NPAR, LIMAX, P) = -sum_g DELG xfac exp(-tau_path) dTAUTOT_LAYINC (leading axis dropped for a
        single model).  dTSURF of this branch is zero."""
        what, W = "cirsradg_ck_transmission", self.dims[0]
        n, L, single, lp, lt, am, tc, dtc = self._layer_args(what, lay_press_pa, lay_temp, amount, taucont, dtaucon, NPAR,
                                                             model_axis="optional")
        NLAYIN, LAYINC, LIMAX, P, SC, _, _ = self._path_args(what, NLAYIN, LAYINC, SCALE, n=n)
        ig = _np(igas_map, np.int32)
        spec = np.empty((n, W, P)); dspec = np.empty((n, W, NPAR, LIMAX, P))
        self._chain_dspec = None
        rc = self._lib.ansfm_cirsradg_ck_transmission(
            self._ctx, n, L, _ptr(lp), _ptr(lt), _ptr(am), _ptr(tc), _ptr(dtc), int(NVMR), int(NPAR), _ptr(ig), P, LIMAX,
            _ptr(NLAYIN), _ptr(LAYINC), _ptr(SC), _ptr(_np(xfac)), _ptr(spec), _ptr(dspec))
        self._check(rc, what)
        return self._gradient_result(single, spec, dspec)

    def _one_model_args(self, what, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map):
        """-> L and the library's arguments L .. igas_map of a fused one-model route"""
        _, L, _, lp, lt, am, tc, dtc = self._layer_args(what, lay_press_pa, lay_temp, amount, taucont, dtaucon, NPAR, model_axis="none")
        return L, (L, _ptr(lp), _ptr(lt), _ptr(am), _ptr(tc), _ptr(dtc), int(NVMR), int(NPAR), _ptr(_np(igas_map, np.int32)))

    def _one_model_paths(self, what, NLAYIN, LAYINC, SCALE, EMTEMP=None, emission=False):
        """-> P and the library's arguments P .. SCALE of a fused one-model route; emission: .. EMTEMP, which is then needed"""
        if emission and EMTEMP is None:
            raise ValueError(what + ": EMTEMP (LIMAX, NPATH) is needed")
        NLAYIN, LAYINC, LIMAX, P, SC, ET, _ = self._path_args(what, NLAYIN, LAYINC, SCALE, EMTEMP)
        return P, (P, LIMAX, _ptr(NLAYIN), _ptr(LAYINC), _ptr(SC)) + ((_ptr(ET),) if emission else ())

    @staticmethod
    def _mix_rows(what, mix, P):
        """The mixing matrix C (Q, P), dense or a triple of compressed rows, as compressed rows: mptr, mpath, mval."""
        if isinstance(mix, tuple):
            mptr, mpath, mval = _np(mix[0], np.int32), _np(mix[1], np.int32).reshape(-1), _np(mix[2]).reshape(-1)
            if mptr.ndim != 1 or mptr.size < 2 or mpath.size != mval.size or mptr[-1] != mpath.size:
                raise ValueError(what + ": mix must be (ptr (Q + 1,), path (nnz,), val (nnz,)) with ptr[-1] = nnz")
            return mptr, mpath, mval
        Cm = _np(mix)
        if Cm.ndim != 2 or Cm.shape[1] != P or Cm.shape[0] < 1:
            raise ValueError(what + ": a dense mix must be (NGEOM, NPATH)")
        nz = Cm != 0.0
        return _np(np.concatenate([[0], np.cumsum(nz.sum(axis=1))]), np.int32), _np(np.nonzero(nz)[1], np.int32), _np(Cm[nz])

    def _mix_args(self, what, mix, P, xfac):
        """-> Q and the library's arguments Q, mix_ptr, mix_path, mix_val, xfac of a route that mixes paths to geometries"""
        mptr, mpath, mval = self._mix_rows(what, mix, P)
        xf = None if xfac is None else _np(xfac).reshape(self.dims[0])
        return mptr.size - 1, (mptr.size - 1, _ptr(mptr), _ptr(mpath), _ptr(mval), _ptr(xf))

    @contextlib.contextmanager
    def _shared_gas_gradient(self, what, dtau_every_gas, L, n=1, only=""):
        """Arms dtau_every_gas (W, L), or nothing for None, for the gradient call made inside the block: a successful call
        consumes it, and leaving the block cancels it if the call failed before that."""
        if dtau_every_gas is None:
            yield
            return
        dg = _np(dtau_every_gas)
        if n != 1 or dg.shape != (self.dims[0], L):
            raise ValueError(what + ": dtau_every_gas must be (NWAVE, NLAY)" + only)
        self._check(self._lib.ansfm_set_shared_gas_gradient(self._ctx, L, _ptr(dg)), "set_shared_gas_gradient")
        try:
            yield
        finally:
            self._lib.ansfm_set_shared_gas_gradient(self._ctx, 0, None)

    @contextlib.contextmanager
    def _phase_variants(self, what, W, phase_of, phasarr_variants):
        """Arms the per-model phase functions (ansfm_set_phase_variants), or nothing for None, for the batched scattering call
        made inside the block.  The library copies the arrays and forgets the setting with the call that meets it; leaving
        the block cancels it if no call was reached."""
        if phase_of is None and phasarr_variants is None:
            yield
            return
        if phase_of is None or phasarr_variants is None:
            raise ValueError(what + ": phase_of and phasarr_variants go together")
        po = np.asarray(phase_of)
        if po.ndim != 1 or po.dtype.kind not in "iu":
            raise ValueError(what + ": phase_of must be an integer array (n_models,)")
        po = _np(po, np.int32)
        pv = _np(phasarr_variants)
        if pv.ndim != 5 or pv.shape[2] != W or pv.shape[3] != 2:
            raise ValueError(what + f": phasarr_variants must be (V - 1, NDUST, NWAVE = {W}, 2, NTHETA), got {pv.shape}")
        if pv.shape[0] == 0:                    # V = 1: variant 0 alone, the plain call
            yield
            return
        self._check(self._lib.ansfm_set_phase_variants(self._ctx, po.shape[0], pv.shape[0] + 1, _ptr(po), pv.shape[1], pv.shape[4],
                                                       _ptr(pv)), "set_phase_variants")
        try:
            yield
        finally:
            self._lib.ansfm_set_phase_variants(self._ctx, 0, 1, None, 0, 0, None)

    def last_scatter_variants(self):
        """((variant, population) pairs whose phase matrices and Hansen factors were formed beside variant 0's, bytes of the
        buffers of variants 1 .. V-1) of the last batched scatter call; (0, 0) without phase variants"""
        a = C.c_int64(); b = C.c_int64()
        self._check(self._lib.ansfm_last_scatter_variants(self._ctx, C.byref(a), C.byref(b), None), "last_scatter_variants")
        return int(a.value), int(b.value)

    def last_scatter_walk_ms(self):
        """milliseconds the phase matrices and the Hansen walk of the last batched scatter call took on the device (variants'
        pairs and their copy included); -1.0 when that call had no such stage of its own (one g-ordinate, model by model)"""
        t = C.c_double()
        self._check(self._lib.ansfm_last_scatter_variants(self._ctx, None, None, C.byref(t)), "last_scatter_variants")
        return float(t.value)

    def _last3(self, fn, what):
        info = (C.c_double * 3)()
        self._check(fn(self._ctx, C.byref(info)), what)
        return int(info[0]), info[1], info[2]

    def cirsradg_ck_transit(self, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map, NLAYIN, LAYINC, SCALE,
                            path_weight, gradients_on_device=False, dtau_every_gas=None):
        """Primary-transit depth with analytic gradients of one model (nemesisPTfm :1838-1995), collapsed over the limb paths
        on the device: AREA (W,) = sum_p path_weight[p] (1 - TRANS[:, p]), TRANS (W, P) the path transmissions, and
        dAREA (W, NPAR, L) = d AREA / d (layer property) with dTAUTOT assembled as in `cirsradg_ck_thermal`.  lay_press_pa,
        lay_temp (L,), amount (NGAS, L), taucont (W, L) or None, dtaucon (W, NPAR, L) or None, NLAYIN (P,), LAYINC / SCALE
        (LIMAX, P), path_weight (P,) the annulus weights c_p (`transit.path_weights`).  gradients_on_device=True: dAREA is not
        copied to the host (None in its place) and `map2pro(None, ...)` with LAYINC = arange(L), NPATH = 1 continues from the
        device copy; only this arms the chain -- after a call that returned dAREA, `map2pro(None, ...)` raises ValueError.  dtau_every_gas as in `cirsradg_ck_thermal`.  NotImplementedError above
        320 layers or paths."""
        what = "cirsradg_ck_transit"
        W = self.dims[0]
        L, layers = self._one_model_args(what, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map)
        P, paths = self._one_model_paths(what, NLAYIN, LAYINC, SCALE)
        cw = _np(path_weight).reshape(P)
        return self._fused_gradient_call(what, L, dtau_every_gas, gradients_on_device, (W, int(NPAR), L),
                                         (*layers, *paths, _ptr(cw)), (np.empty(W), np.empty((W, P))))

    def transit_last(self):
        """(scratch bytes beyond the gas stage, k_transit_sens ms, k_transit_grad ms) of the last cirsradg_ck_transit call"""
        return self._last3(self._lib.ansfm_transit_last, "transit_last")

    def cirsradg_ck_occultation(self, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map, NLAYIN, LAYINC, SCALE,
                                mix, xfac=None, gradients_on_device=False, dtau_every_gas=None):
        """Solar occultation with analytic gradients of one model (nemesisSOfmg :983-1249), the limb paths mixed to the
        geometries on the device: MOD (W, Q) = xfac * TRANS @ C.T, TRANS (W, P) the path transmissions, and dMOD (W, NPAR, L, Q)
        = d MOD / d (layer property), in the layout of the reference's dSPECOUT with the layers in place of the path entries and
        the geometries in place of the paths; dTAUTOT assembled as in `cirsradg_ck_thermal`.  mix: the mixing matrix C, dense
        (Q, P) (its zeros are dropped) or a triple (ptr (Q + 1,), path (nnz,), val (nnz,)) of compressed rows
        (`occultation.tangent_mix`); a geometry with an empty row gives zeros.  The other arguments as `cirsradg_ck_transit`;
        xfac (W,) the solar flux or None.  gradients_on_device=True: dMOD is not copied to the host (None in its place) and
        `map2pro(None, ...)` with NPATH = Q, NLAYIN = [L] * Q, LAYINC[:, q] = arange(L) continues from the device copy; only this
        arms the chain.  dMOD takes 8 W NPAR L Q bytes on the device.  NotImplementedError above 320 layers or paths, or when
        dMOD cannot be reserved."""
        what = "cirsradg_ck_occultation"
        W = self.dims[0]
        L, layers = self._one_model_args(what, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map)
        P, paths = self._one_model_paths(what, NLAYIN, LAYINC, SCALE)
        Q, mixing = self._mix_args(what, mix, P, xfac)
        return self._fused_gradient_call(what, L, dtau_every_gas, gradients_on_device, (W, int(NPAR), L, Q),
                                         (*layers, *paths, *mixing), (np.empty((W, Q)), np.empty((W, P))))

    def occultation_last(self):
        """(scratch bytes beyond the gas stage and dMOD, k_occ_paths ms, k_occ_grad ms) of the last cirsradg_ck_occultation call"""
        return self._last3(self._lib.ansfm_occultation_last, "occultation_last")

    def cirsradg_ck_limb(self, ISPACE, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map, NLAYIN, LAYINC, SCALE,
                         EMTEMP, mix, xfac=None, gradients_on_device=False, dtau_every_gas=None):
        """Limb thermal emission with analytic gradients of one model (nemesisLfmg :1372-1521), the limb paths mixed to the
        geometries on the device: MOD (W, Q) = xfac * SPEC @ C.T, SPEC (W, P) the path radiances before xfac, and
        dMOD (W, NPAR, L, Q) = d MOD / d (layer property), in the layout of the reference's dSPECOUT with the layers in place of
        the path entries and the geometries in place of the paths; dTAUTOT assembled as in `cirsradg_ck_thermal`.  EMTEMP
        (LIMAX, P) as SCALE; mix, xfac, gradients_on_device and dtau_every_gas as `cirsradg_ck_occultation` takes them
        (`limb.tangent_mix`); xfac (W,) the factor of :4158-4168 or None.  dMOD takes 8 W NPAR L Q bytes on the device.
        NotImplementedError above 160 layers, for a path that ends at the lower boundary (limb paths only), or when dMOD or the
        scratch cannot be reserved."""
        what = "cirsradg_ck_limb"
        W = self.dims[0]
        L, layers = self._one_model_args(what, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map)
        P, paths = self._one_model_paths(what, NLAYIN, LAYINC, SCALE, EMTEMP, emission=True)
        Q, mixing = self._mix_args(what, mix, P, xfac)
        return self._fused_gradient_call(what, L, dtau_every_gas, gradients_on_device, (W, int(NPAR), L, Q),
                                         (int(ISPACE), *layers, *paths, *mixing), (np.empty((W, Q)), np.empty((W, P))))

    def limb_last(self):
        """(scratch bytes beyond the gas stage and dMOD, k_limb_planck + k_limb_sens ms, k_limb_grad ms) of the last
        cirsradg_ck_limb call"""
        return self._last3(self._lib.ansfm_limb_last, "limb_last")

    def cirsradg_ck_disc(self, ISPACE, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map, LAYINC, SCALE, EMTEMP,
                         TSURF, EMISSIVITY=None, mix=None, xfac=None, gradients_on_device=False, dtau_every_gas=None):
        """Disc-averaged thermal emission with analytic gradients of one model (nemesisdiscfmg :1719-1834), the averaging points
        mixed to the geometries on the device.  The points are P paths through ONE layer sequence: LAYINC (N,), EMTEMP (N,),
        SCALE (N, P); unlike `cirsradg_ck_limb` the sequence may end at the lower boundary, with TSURF and EMISSIVITY (W,) as
        `cirsradg_ck_thermal` takes them (:6479-6498).  Returns MOD (W, Q) = xfac * SPEC @ C.T, SPEC (W, P) the path radiances
        before xfac, dTSMOD (W, Q) = xfac * sum_p C[q, p] dTSURF_p and dMOD (W, NPAR, L, Q) in the layout of `cirsradg_ck_limb`.
        mix (`disc.average_mix`), xfac, gradients_on_device and dtau_every_gas as `cirsradg_ck_limb` takes them.  dMOD takes
        8 W NPAR L Q bytes on the device.  ValueError for TSURF > 0 without EMISSIVITY, a LAYINC outside the layers or a bad mix;
        NotImplementedError above 160 layers or when dMOD or the scratch cannot be reserved."""
        what = "cirsradg_ck_disc"
        W = self.dims[0]
        L, layers = self._one_model_args(what, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map)
        LAYINC = _np(LAYINC, np.int32).reshape(-1)
        N = LAYINC.shape[0]
        ET = _np(EMTEMP).reshape(-1)
        SC = _np(SCALE)
        if SC.ndim == 1:
            SC = _np(SC[:, None])
        if N < 1 or SC.ndim != 2 or SC.shape[0] != N or SC.shape[1] < 1 or ET.shape[0] != N:
            raise ValueError(what + ": LAYINC (N,), EMTEMP (N,) and SCALE (N, NPATH) with N, NPATH >= 1")
        P = SC.shape[1]
        if mix is None:
            raise ValueError(what + ": mix is required (disc.average_mix)")
        Q, mixing = self._mix_args(what, mix, P, xfac)
        em = None if EMISSIVITY is None else _np(EMISSIVITY).reshape(W)
        return self._fused_gradient_call(
            what, L, dtau_every_gas, gradients_on_device, (W, int(NPAR), L, Q),
            (int(ISPACE), *layers, N, _ptr(LAYINC), _ptr(ET), P, _ptr(SC), float(TSURF), _ptr(em), *mixing),
            (np.empty((W, Q)), np.empty((W, P)), np.empty((W, Q))))

    def disc_last(self):
        """(scratch bytes beyond the gas stage and dMOD, k_disc_planck + k_disc_sens ms, k_disc_grad ms) of the last
        cirsradg_ck_disc call"""
        return self._last3(self._lib.ansfm_disc_last, "disc_last")

    def cirsradg_ck_thermal(self, ISPACE, lay_press_pa, lay_temp, amount, taucont, dtaucon, NVMR, NPAR, igas_map,
                            NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY=None, xfac=None, gradients_on_device=False,
                            dtau_every_gas=None):
        """CIRSrad(return_grad=True): returns SPECOUT (n,W,P), dSPECOUT (n,W,NPAR,LIMAX,P), dTSURF (n,W,P)
        (leading axis dropped for a single model).  gradients_on_device (single model): dSPECOUT is not copied to the host
        (None is returned in its place); `map2pro(None, ...)` takes it from the device.  dtau_every_gas (W, L), single
        model: added to dTAUCON of every gas parameter (the Rayleigh term, :3955-3957) without building the NVMR copies."""
        what, W = "cirsradg_ck_thermal", self.dims[0]
        n, L, single, lp, lt, am, tc, dtc = self._layer_args(what, lay_press_pa, lay_temp, amount, taucont, dtaucon, NPAR,
                                                             model_axis="optional")
        NLAYIN, LAYINC, LIMAX, P, SC, ET, TS = self._path_args(what, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, n)
        ig = _np(igas_map, np.int32)
        on_dev = bool(gradients_on_device) and n == 1
        spec = np.empty((n, W, P)); dts = np.empty((n, W, P))
        dspec = None if on_dev else np.empty((n, W, NPAR, LIMAX, P))
        with self._shared_gas_gradient(what, dtau_every_gas, L, n, " for a single model"):
            self._chain_dspec = None
            rc = self._lib.ansfm_cirsradg_ck_thermal(
                self._ctx, int(ISPACE), n, L, _ptr(lp), _ptr(lt), _ptr(am), _ptr(tc), _ptr(dtc), int(NVMR), int(NPAR),
                _ptr(ig), P, LIMAX, _ptr(NLAYIN), _ptr(LAYINC), _ptr(SC), _ptr(ET), _ptr(TS), _ptr(_np(EMISSIVITY)),
                _ptr(_np(xfac)), _ptr(spec), _ptr(dspec), _ptr(dts))
        self._check(rc, what)
        return self._gradient_result(single, spec, dspec, dts, (W, int(NPAR), LIMAX, P) if on_dev else None)

    def cirsradg_ck_thermal_cont(self, ISPACE, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, NVMR, NPAR,
                                 igas_map, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY=None, xfac=None,
                                 gradients_on_device=False, variant=None):
        """`cirsradg_ck_thermal` with the continuum and its gradients (dTAUCON of calculate_layer_opacity :3940-3981) formed
        inside the call from the resident sources (upload_cia, upload_dust) and the Rayleigh parametrisations, in place of
        taucont / dtaucon / dtau_every_gas: q (n, L, NVMR) = PP / PRESS with FRAC, DELH (n, L) switch CIA on (None: off); CONT
        (n, L, NDUST) switches the aerosols on (None: off); IRAY 0 or as in calc_tau_rayleigh with f4 (n, L, 4) (rayleigh_f4) for
        IRAY 4; TOTAM (n, L) for CIA and Rayleigh.  Host arrays, the leading axis optional for one model.  Same bits as
        calc_tau_cia(with_grad=True) + calc_tau_dust + calc_tau_rayleigh assembled on the host and passed to
        `cirsradg_ck_thermal`.  Returns what that returns; gradients_on_device as there.  ValueError for a source that is not
        resident, an NVMR other than the CIA source's, an NPAR other than NVMR + 2 + the aerosol source's NDUST;
        NotImplementedError for NVMR > 46."""
        what = "cirsradg_ck_thermal_cont"
        W = self.dims[0]
        n, L, single, lp, lt, am, _, _ = self._layer_args(what, lay_press_pa, lay_temp, amount, model_axis="optional")
        NVMR, NPAR = int(NVMR), int(NPAR)
        opt = lambda a, shape: None if a is None else _np(a).reshape(shape)
        cont, _ = self._fused_cont_args(what, n, L, opt(q, (n, L, NVMR)), opt(FRAC, (n, L)), opt(TOTAM, (n, L)), opt(DELH, (n, L)),
                                        opt(CONT, (n, L, -1)), IRAY, opt(f4, (n, L, 4)), variant, ncont=getattr(self, "dust_n", None))
        NLAYIN, LAYINC, LIMAX, P, SC, ET, TS = self._path_args(what, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, n)
        ig = _np(igas_map, np.int32)
        on_dev = bool(gradients_on_device) and n == 1
        spec = np.empty((n, W, P)); dts = np.empty((n, W, P))
        dspec = None if on_dev else np.empty((n, W, NPAR, LIMAX, P))
        self._chain_dspec = None
        rc = self._lib.ansfm_cirsradg_ck_thermal_cont(
            self._ctx, int(ISPACE), n, L, _ptr(lp), _ptr(lt), _ptr(am), *cont, NVMR, NPAR, _ptr(ig), P, LIMAX, _ptr(NLAYIN),
            _ptr(LAYINC), _ptr(SC), _ptr(ET), _ptr(TS), _ptr(_np(EMISSIVITY)), _ptr(_np(xfac)), _ptr(spec), _ptr(dspec), _ptr(dts))
        self._check(rc, what)
        return self._gradient_result(single, spec, dspec, dts, (W, NPAR, LIMAX, P) if on_dev else None)

    def cirsradg_ck_thermal_cont_dev(self, ISPACE, n_models, L, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH, CONT, IRAY, f4,
                                     NVMR, NPAR, igas_map, P, LIMAX, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, xfac, SPECOUT,
                                     dSPECOUT, dTSURF, variant=None):
        """`cirsradg_ck_thermal_cont` on contiguous float64 torch device tensors (igas_map: a host array; NLAYIN, LAYINC int32
        tensors); asynchronous.  q, FRAC, TOTAM, DELH, CONT, f4 as `cirsrad_ck_thermal_cont_dev` takes them, with the same shape
        checks; SPECOUT (n, W, P), dSPECOUT (n, W, NPAR, LIMAX, P), dTSURF (n, W, P) are filled."""
        what = "cirsradg_ck_thermal_cont_dev"
        cont, _ = self._fused_cont_args(what, n_models, L, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, variant, dev=True,
                                        ncont=getattr(self, "dust_n", -1))
        W = self.dims[0]
        for a, shape in ((SPECOUT, (n_models, W, P)), (dSPECOUT, (n_models, W, int(NPAR), LIMAX, P)), (dTSURF, (n_models, W, P))):
            if a is None or tuple(a.shape) != shape or not a.is_contiguous():
                raise ValueError(what + ": the outputs must be contiguous tensors, here of shape %s" % (shape,))
        ig = _np(igas_map, np.int32)
        self._chain_dspec = None
        rc = self._lib.ansfm_cirsradg_ck_thermal_cont_dev(
            self._ctx, int(ISPACE), int(n_models), int(L), _ptr(lay_press_pa), _ptr(lay_temp), _ptr(amount), *cont, int(NVMR), int(NPAR),
            _ptr(ig), int(P), int(LIMAX), _ptr(NLAYIN), _ptr(LAYINC), _ptr(SCALE), _ptr(EMTEMP), _ptr(TSURF), _ptr(EMISSIVITY),
            _ptr(xfac), _ptr(SPECOUT), _ptr(dSPECOUT), _ptr(dTSURF))
        self._check(rc, what)

    def cirsrad_ck_thermal_dev(self, ISPACE, n_models, L, lay_press_pa, lay_temp, amount, taucont, P, LIMAX,
                               NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, SOLFLUX, REFLECTANCE, SOL_ANG,
                               EMISS_ANG, xfac, SPECOUT):
        """All arguments torch device tensors (or None where optional); asynchronous."""
        rc = self._lib.ansfm_cirsrad_ck_thermal_dev(
            self._ctx, int(ISPACE), int(n_models), int(L), _ptr(lay_press_pa), _ptr(lay_temp), _ptr(amount),
            _ptr(taucont), int(P), int(LIMAX), _ptr(NLAYIN), _ptr(LAYINC), _ptr(SCALE), _ptr(EMTEMP), _ptr(TSURF),
            _ptr(EMISSIVITY), _ptr(SOLFLUX), _ptr(REFLECTANCE), _ptr(SOL_ANG), _ptr(EMISS_ANG), _ptr(xfac),
            _ptr(SPECOUT))
        self._check(rc, "cirsrad_ck_thermal_dev")

    def cirsrad_ck_thermal_ray_dev(self, ISPACE, n_models, L, lay_press_pa, lay_temp, amount, IRAY, TOTAM, f4, P, LIMAX,
                                   NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, SOLFLUX, REFLECTANCE, SOL_ANG,
                                   EMISS_ANG, xfac, SPECOUT, variant=None):
        """cirsrad_ck_thermal_dev for a batch whose continuum is Rayleigh scattering alone: TOTAM (n, L) and, IRAY 4,
        f4 (n, L, 4) (see rayleigh_f4) are device tensors; the continuum is formed per distinct layer inside the call."""
        rc = self._lib.ansfm_cirsrad_ck_thermal_ray_dev(
            self._ctx, int(ISPACE), int(n_models), int(L), _ptr(lay_press_pa), _ptr(lay_temp), _ptr(amount),
            _ray_mode(IRAY, variant), _ptr(TOTAM), _ptr(f4), int(P), int(LIMAX), _ptr(NLAYIN), _ptr(LAYINC), _ptr(SCALE),
            _ptr(EMTEMP), _ptr(TSURF), _ptr(EMISSIVITY), _ptr(SOLFLUX), _ptr(REFLECTANCE), _ptr(SOL_ANG), _ptr(EMISS_ANG),
            _ptr(xfac), _ptr(SPECOUT))
        self._check(rc, "cirsrad_ck_thermal_ray_dev")

    def cirsrad_ck_thermal_cont_dev(self, ISPACE, n_models, L, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH, CONT, IRAY,
                                    f4, P, LIMAX, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMISSIVITY, SOLFLUX, REFLECTANCE,
                                    SOL_ANG, EMISS_ANG, xfac, SPECOUT, variant=None):
        """cirsrad_ck_thermal_dev for a batch whose continuum is (TAUCIA + TAUDUST) + TAURAY from the resident sources
        (upload_cia, upload_dust), formed per distinct layer inside the call.  Contiguous float64 device tensors: q (n, L,
        NVMR) = PP / PRESS with FRAC, DELH (n, L) switch CIA on (None: off); CONT (n, L, NDUST) after any
        DUST_RENORMALISATION switches the aerosols on (None: off); IRAY 0 or as in cirsrad_ck_thermal_ray_dev with f4 (n,
        L, 4); TOTAM (n, L) for CIA and Rayleigh."""
        cont, _ = self._fused_cont_args("cirsrad_ck_thermal_cont_dev", n_models, L, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, variant, dev=True,
                                        ncont=getattr(self, "dust_n", -1))
        rc = self._lib.ansfm_cirsrad_ck_thermal_cont_dev(
            self._ctx, int(ISPACE), int(n_models), int(L), _ptr(lay_press_pa), _ptr(lay_temp), _ptr(amount), *cont, int(P), int(LIMAX),
            _ptr(NLAYIN), _ptr(LAYINC), _ptr(SCALE), _ptr(EMTEMP), _ptr(TSURF), _ptr(EMISSIVITY), _ptr(SOLFLUX), _ptr(REFLECTANCE),
            _ptr(SOL_ANG), _ptr(EMISS_ANG), _ptr(xfac), _ptr(SPECOUT))
        self._check(rc, "cirsrad_ck_thermal_cont_dev")

    @staticmethod
    def rayleigh_f4(ID, ISO, VMR):
        """calc_tau_rayleighls' composition (:5748-5767): VMR (..., NVMR) numpy array or torch tensor -> (..., 4) mixing
        ratios of H2, He, CH4, NH3, zero where the gas is absent; the last matching gas wins."""
        ID = np.asarray(ID); ISO = np.asarray(ISO)
        if isinstance(VMR, np.ndarray):
            f4 = np.zeros(VMR.shape[:-1] + (4,))
        else:
            import torch
            f4 = torch.zeros(tuple(VMR.shape[:-1]) + (4,), dtype=VMR.dtype, device=VMR.device)
        for j in range(ID.size):
            if ISO[j] in (0, 1):
                col = {39: 0, 40: 1, 6: 2, 11: 3}.get(int(ID[j]))
                if col is not None:
                    f4[..., col] = VMR[..., j]
        return f4

    def scloud11wave_core(self, phasarr, radg, sol_angs, emiss_angs, solar, aphis, lowbc, brdf_matrix, mu1, wt1, nf,
                          vwaves, bnu, taus, tauray, omegas_s, nphi, iray, imie, lfrac):
        """Multiple_Scattering_Core.scloud11wave_core (same arguments) -> rad (NPATH, NG, NWAVE)."""
        phasarr = _np(phasarr); taus = _np(taus)
        ncont, nwave, _, nth = phasarr.shape
        nmu = len(mu1); ngeom = len(emiss_angs)
        _, ng, nlay = taus.shape
        if ngeom > self.MS_PATHS_PER_CALL:      # the chain kernels keep one path per lane of a 16-lane row: groups of paths
            emi = np.asarray(emiss_angs, dtype=float)
            if not (np.all(emi < 90) or np.all(emi > 90)):
                raise ValueError("scloud11wave_core: INVALID: Emission angles are a mix of values above and below 90 degrees.")
            parts = [self.scloud11wave_core(phasarr, radg, np.asarray(sol_angs)[g], emi[g], solar, np.asarray(aphis)[g], lowbc,
                                            brdf_matrix, mu1, wt1, nf, vwaves, bnu, taus, tauray, omegas_s, nphi, iray, imie, lfrac)
                     for g in self._path_groups(ngeom)]
            return np.concatenate(parts, axis=0)
        rad = np.empty((ngeom, ng, nwave))
        rc = self._lib.ansfm_scloud11wave_core(
            self._ctx, ncont, nwave, nth, _ptr(phasarr), _ptr(_np(radg)), ngeom, _ptr(_np(sol_angs)),
            _ptr(_np(emiss_angs)), _ptr(_np(solar)), _ptr(_np(aphis)), int(lowbc), _ptr(_np(brdf_matrix)), nmu,
            _ptr(_np(mu1)), _ptr(_np(wt1)), int(nf), _ptr(_np(bnu)), ng, nlay, _ptr(taus), _ptr(_np(tauray)),
            _ptr(_np(omegas_s)), int(nphi), int(iray), int(imie), _ptr(_np(lfrac)), _ptr(rad))
        self._check(rc, "scloud11wave_core")
        return rad

    MS_PATHS_PER_CALL = 16

    def _path_groups(self, ngeom):
        n = self.MS_PATHS_PER_CALL
        return [slice(i, min(i + n, ngeom)) for i in range(0, ngeom, n)]

    @staticmethod
    def _scatter_common(phasarr, sol_angs, emiss_angs, aphis, mu1):
        """What the scattering wrappers share -> ((phasarr or None, ncont, nth), (sol, emi, aph, P), (mu1, nmu))"""
        phasarr = None if phasarr is None else _np(phasarr)
        ncont, nth = (0, 0) if phasarr is None else (phasarr.shape[0], phasarr.shape[3])
        sol = _np(np.atleast_1d(sol_angs)); emi = _np(np.atleast_1d(emiss_angs)); aph = _np(np.atleast_1d(aphis))
        mu1 = _np(mu1)
        return (phasarr, ncont, nth), (sol, emi, aph, sol.shape[0]), (mu1, mu1.shape[0])

    def _scatter_batch_common(self, what, lay_press_pa, lay_temp, amount, phasarr, radg, sol_angs, emiss_angs, aphis, mu1,
                              wave_slice, whole_axis=True):
        """What the batched scattering entries share -> W, (n, L, lp, lt, am), the three groups of `_scatter_common`, radg,
        (W_full, w_begin).  The layers carry a model axis; radg holds n NWAVE NMU values; phasarr covers the axis wave_slice =
        (w_begin, W_full) names -- the table's own without one, where whole_axis=False leaves that to the library."""
        dims, _ = self.ktable_info()
        W = dims[0]
        n, L, _, lp, lt, am, _, _ = self._layer_args(what, lay_press_pa, lay_temp, amount, model_axis="required", dims=dims)
        phase, geom, (mu1, nmu) = self._scatter_common(phasarr, sol_angs, emiss_angs, aphis, mu1)
        rg = _np(radg)
        if rg.size != n * W * nmu:
            raise ValueError(f"{what}: radg must be (n_models, NWAVE, NMU)")
        w_begin, W_full = (0, W) if wave_slice is None else (int(v) for v in wave_slice)
        if phase[0] is not None and (whole_axis or wave_slice is not None) and phase[0].shape[1] != W_full:
            raise ValueError(f"{what}: phasarr must cover the whole axis (NDUST, W_full, 2, NTHETA)")
        return W, (n, L, lp, lt, am), phase, geom, (mu1, nmu), rg, (W_full, w_begin)

    def cirsrad_ck_scatter(self, ISPACE, lay_press_pa, lay_temp, amount, TAUCIA, TAUDUST, TAURAY, TAUSCAT, phasarr, lfrac,
                           radg, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, mu1, wt1, nf, nphi, iray, imie,
                           xfac=None, return_spec_g=False):
        """CIRSrad, scattering branch (ForwardModel_0.py:4478-4501, :4343, scloud11wave :5018-5165) on the uploaded k-table:
        vertical gas opacities, TAUTOT, OMEGA and BB are formed in HBM and go straight into the doubling / adding kernels.
        TAUCIA / TAUDUST / TAURAY / TAUSCAT (NWAVE, NLAY) or None; phasarr (NDUST, NWAVE, 2, NTHETA) and lfrac (NWAVE, NDUST,
        NLAY) as scloud11wave_core takes them -> SPECOUT (NWAVE, NPATH) [, SPEC (NWAVE, NG, NPATH)]."""
        dims, _ = self.ktable_info()
        W, G, S = dims[0], dims[1], dims[4]
        lay_press_pa = _np(lay_press_pa); L = lay_press_pa.shape[0]
        amount = _np(amount)
        if amount.shape != (S, L):
            raise ValueError("amount must be (NGAS, NLAY)")
        wl = lambda a: None if a is None else _np(a).reshape(W, L)
        (phasarr, ncont, nth), (sol, emi, aph, P), (mu1, nmu) = self._scatter_common(phasarr, sol_angs, emiss_angs, aphis, mu1)
        if P > self.MS_PATHS_PER_CALL:          # more paths than one call takes: groups of paths, the chains of each re-run
            if not (np.all(emi < 90) or np.all(emi > 90)):
                raise ValueError("cirsrad_ck_scatter: INVALID: Emission angles are a mix of values above and below 90 degrees.")
            parts = [self.cirsrad_ck_scatter(ISPACE, lay_press_pa, lay_temp, amount, TAUCIA, TAUDUST, TAURAY, TAUSCAT, phasarr, lfrac,
                                             radg, sol[g], emi[g], aph[g], solar, lowbc, brdf_matrix, mu1, wt1, nf, nphi, iray, imie,
                                             xfac=xfac, return_spec_g=return_spec_g) for g in self._path_groups(P)]
            if return_spec_g:
                return np.concatenate([p_[0] for p_ in parts], axis=1), np.concatenate([p_[1] for p_ in parts], axis=2)
            return np.concatenate(parts, axis=1)
        out = np.empty((W, P)); spec_g = np.empty((W, G, P)) if return_spec_g else None
        rc = self._lib.ansfm_cirsrad_ck_scatter(
            self._ctx, int(ISPACE), L, _ptr(lay_press_pa), _ptr(_np(lay_temp)), _ptr(amount), _ptr(wl(TAUCIA)), _ptr(wl(TAUDUST)),
            _ptr(wl(TAURAY)), _ptr(wl(TAUSCAT)), ncont, nth, _ptr(phasarr), _ptr(_np(lfrac)), _ptr(_np(radg)), P, _ptr(sol),
            _ptr(emi), _ptr(aph), _ptr(_np(solar)), int(lowbc), _ptr(_np(brdf_matrix)), nmu, _ptr(mu1), _ptr(_np(wt1)), int(nf),
            int(nphi), int(iray), int(imie), _ptr(_np(xfac)), _ptr(out), _ptr(spec_g))
        self._check(rc, "cirsrad_ck_scatter")
        return (out, spec_g) if return_spec_g else out

    def cirsrad_ck_scatter_batch(self, ISPACE, lay_press_pa, lay_temp, amount, TAUCIA, TAUDUST, TAURAY, TAUSCAT, phasarr, lfrac,
                                 radg, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, mu1, wt1, nf, nphi, iray, imie,
                                 xfac=None, wave_slice=None, phase_of=None, phasarr_variants=None):
        """The scattering branch of CIRSrad for the n forward models of a numerical Jacobian (ansfm_cirsrad_ck_scatter_batch):
        lay_press_pa / lay_temp (n, NLAY), amount (n, NGAS, NLAY), TAUCIA / TAUDUST / TAURAY / TAUSCAT (n, NWAVE, NLAY) or None,
        lfrac (n, NWAVE, NDUST, NLAY), radg (n, NWAVE, NMU); the rest as `cirsrad_ck_scatter` -> SPECOUT (n, NWAVE, NPATH).
        Layers whose inputs equal model 0's are taken from model 0's doubling results (`last_scatter_cache()`).

        wave_slice = (w_begin, W_full): the uploaded table is the slice [w_begin, w_begin + NWAVE) of a W_full axis
        (ansfm_cirsrad_ck_scatter_batch_slice).  phasarr then covers the whole axis, (NDUST, W_full, 2, NTHETA); every other
        per-wavenumber input and the result cover the slice.  The slices side by side equal the call over the whole axis, bit
        for bit.

        phase_of (n,) int and phasarr_variants (V - 1, NDUST, NWAVE, 2, NTHETA): per-model phase functions
        (ansfm_set_phase_variants).  Model m runs with variant phase_of[m]; variant 0 is phasarr and phase_of[0] must be 0.
        Every spectrum has the bits of `cirsrad_ck_scatter` with that model's phase function; a layer stays model 0's where none
        of the changed populations is present (lfrac == 0).  Whole axis and more than one g-ordinate only: NotImplementedError
        with wave_slice or an LBL table, and when the variants' buffers find no room."""
        what = "cirsrad_ck_scatter_batch"
        W, (n, L, lp, lt, am), (phasarr, ncont, nth), (sol, emi, aph, P), (mu1, nmu), rg, axis = self._scatter_batch_common(
            what, lay_press_pa, lay_temp, amount, phasarr, radg, sol_angs, emiss_angs, aphis, mu1, wave_slice, whole_axis=False)
        nwl = lambda a: None if a is None else _np(a).reshape(n, W, L)
        lf = None if lfrac is None else _np(lfrac).reshape(n, W, ncont, L)
        out = np.empty((n, W, P))
        args = (self._ctx, int(ISPACE), n, L, _ptr(lp), _ptr(lt), _ptr(am), _ptr(nwl(TAUCIA)),
                _ptr(nwl(TAUDUST)), _ptr(nwl(TAURAY)), _ptr(nwl(TAUSCAT)), ncont, nth, _ptr(phasarr), _ptr(lf), _ptr(rg), P, _ptr(sol),
                _ptr(emi), _ptr(aph), _ptr(_np(solar)), int(lowbc), _ptr(_np(brdf_matrix)), nmu, _ptr(mu1), _ptr(_np(wt1)), int(nf),
                int(nphi), int(iray), int(imie), _ptr(_np(xfac)), _ptr(out))
        with self._phase_variants(what, W, phase_of, phasarr_variants):
            if wave_slice is None:
                self._check(self._lib.ansfm_cirsrad_ck_scatter_batch(*args), what)
            else:
                self._check(self._lib.ansfm_cirsrad_ck_scatter_batch_slice(*args, *axis), what + "_slice")
        return out

    def cirsrad_ck_scatter_batch_rows(self, ISPACE, lay_press_pa, lay_temp, amount, cont_row, TAUCIA_rows, TAUDUST_rows, TAURAY_rows,
                                      TAUSCAT_rows, phasarr, lfrac_rows, radg, sol_angs, emiss_angs, aphis, solar, lowbc,
                                      brdf_matrix, mu1, wt1, nf, nphi, iray, imie, xfac=None, wave_slice=None, phase_of=None,
                                      phasarr_variants=None):
        """`cirsrad_ck_scatter_batch` with the continuum once per distinct layer (ansfm_cirsrad_ck_scatter_batch_rows):
        cont_row (n, NLAY) int, the continuum row of every (model, layer); TAUCIA_rows / TAUDUST_rows / TAURAY_rows / TAUSCAT_rows
        (R, NWAVE) or None and lfrac_rows (R, NDUST, NWAVE), wavenumber fastest (`continuum_rows.ContinuumRows` packs them).
        The rest, wave_slice included, as `cirsrad_ck_scatter_batch` -> SPECOUT (n, NWAVE, NPATH), bit-identical to that call
        with the expanded arrays.  A layer is taken from model 0's doubling results when its gas inputs are model 0's and
        cont_row[m, l] == cont_row[0, l] -- and, with phase_of / phasarr_variants (as in `cirsrad_ck_scatter_batch`), when the
        layer's lfrac row is 0 for every population whose phase function differs from model 0's."""
        what = "cirsrad_ck_scatter_batch_rows"
        W, (n, L, lp, lt, am), (phasarr, ncont, nth), (sol, emi, aph, P), (mu1, nmu), rg, axis = self._scatter_batch_common(
            what, lay_press_pa, lay_temp, amount, phasarr, radg, sol_angs, emiss_angs, aphis, mu1, wave_slice)
        cr = np.asarray(cont_row)
        if cr.shape != (n, L) or cr.dtype.kind not in "iu":
            raise ValueError("cont_row must be an integer array (n_models, NLAY)")
        cr = _np(cr, np.int32)
        rows = [None if a is None else _np(a) for a in (TAUCIA_rows, TAUDUST_rows, TAURAY_rows, TAUSCAT_rows)]
        lf = None if lfrac_rows is None or ncont == 0 else _np(lfrac_rows)
        if ncont > 0 and lf is None:
            raise ValueError("lfrac_rows is needed with aerosols (phasarr given)")
        R = next((a.shape[0] for a in rows + [lf] if a is not None and a.ndim >= 1), max(int(cr.max()) + 1, 1))   # no array at all: any R serves
        for name, a in zip(("TAUCIA_rows", "TAUDUST_rows", "TAURAY_rows", "TAUSCAT_rows"), rows):
            if a is not None and a.shape != (R, W):
                raise ValueError(f"{name} must be (R, NWAVE) = ({R}, {W}), got {a.shape}")
        if lf is not None and lf.shape != (R, ncont, W):
            raise ValueError(f"lfrac_rows must be (R, NDUST, NWAVE) = ({R}, {ncont}, {W}), got {lf.shape}")
        out = np.empty((n, W, P))
        with self._phase_variants(what, W, phase_of, phasarr_variants):
            rc = self._lib.ansfm_cirsrad_ck_scatter_batch_rows(
                self._ctx, int(ISPACE), n, L, _ptr(lp), _ptr(lt), _ptr(am), int(R), _ptr(cr), _ptr(rows[0]), _ptr(rows[1]), _ptr(rows[2]),
                _ptr(rows[3]), ncont, nth, _ptr(phasarr), _ptr(lf), _ptr(rg), P, _ptr(sol), _ptr(emi), _ptr(aph), _ptr(_np(solar)),
                int(lowbc), _ptr(_np(brdf_matrix)), nmu, _ptr(mu1), _ptr(_np(wt1)), int(nf), int(nphi), int(iray), int(imie),
                _ptr(_np(xfac)), _ptr(out), *axis)
            self._check(rc, what)
        return out

    def cirsrad_ck_scatter_batch_cont(self, ISPACE, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, phasarr,
                                      radg, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, mu1, wt1, nf, nphi, iray, imie,
                                      xfac=None, wave_slice=None, variant=None):
        """`cirsrad_ck_scatter_batch_rows` with the rows formed inside the call from the resident sources (upload_cia,
        upload_dust) and the Rayleigh parametrisations (ansfm_cirsrad_ck_scatter_batch_cont): q (n, NLAY, NVMR) = PP / PRESS
        with FRAC, DELH (n, NLAY) switch CIA on (None: off); CONT (n, NLAY, NDUST) after any DUST_RENORMALISATION switches the
        aerosols on (None: off; NDUST as uploaded = phasarr.shape[0]); IRAY 0, 1, 2 or 4 (variant='v': calc_tau_rayleighv) with
        f4 (n, NLAY, 4) for IRAY 4 (`rayleigh_f4`); TOTAM (n, NLAY) for CIA and Rayleigh.  Host arrays.  The rest, wave_slice
        included, as `cirsrad_ck_scatter_batch_rows` -> SPECOUT (n, NWAVE, NPATH), bit-identical to that call on the rows of
        calc_tau_cia / calc_tau_dust / calc_tau_rayleigh."""
        return self._scatter_cont("cirsrad_ck_scatter_batch_cont", ISPACE, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH, CONT,
                                  IRAY, f4, phasarr, None, None, radg, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, mu1, wt1,
                                  nf, nphi, iray, imie, xfac, wave_slice, variant)

    def cirsrad_ck_scatter_batch_src(self, ISPACE, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, theta_deg,
                                     radg, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, mu1, wt1, nf, nphi, iray, imie,
                                     xfac=None, wave_slice=None, variant=None):
        """`cirsrad_ck_scatter_batch_cont` with phasarr formed on the device from the resident phase-function source
        (upload_phase; ansfm_cirsrad_ck_scatter_batch_src): theta_deg (NTHETA,) is Scatter.THETA, ascending; row 1 is
        np.cos(theta_deg * pi / 180), formed here.  Whole axis only.  Bit-identical to the `_cont` call with
        `phasarr_from_source(theta_deg)`."""
        theta = _np(np.atleast_1d(theta_deg))
        return self._scatter_cont("cirsrad_ck_scatter_batch_src", ISPACE, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH, CONT,
                                  IRAY, f4, None, theta, _np(np.cos(theta * np.pi / 180)), radg, sol_angs, emiss_angs, aphis, solar,
                                  lowbc, brdf_matrix, mu1, wt1, nf, nphi, iray, imie, xfac, wave_slice, variant)

    def _scatter_cont(self, what, ISPACE, lay_press_pa, lay_temp, amount, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, phasarr, theta, mu_theta,
                      radg, sol_angs, emiss_angs, aphis, solar, lowbc, brdf_matrix, mu1, wt1, nf, nphi, iray, imie, xfac, wave_slice,
                      variant):
        """the `_cont` entry (phasarr) or the `_src` entry (theta, mu_theta)"""
        W, (n, L, lp, lt, am), (phasarr, npop, nth), (sol, emi, aph, P), (mu1, nmu), rg, axis = self._scatter_batch_common(
            what, lay_press_pa, lay_temp, amount, phasarr, radg, sol_angs, emiss_angs, aphis, mu1, wave_slice)
        if theta is not None:                   # the populations are those of the aerosol columns
            npop, nth = None, theta.shape[0]
        elif npop > 0 and CONT is None:
            raise ValueError(f"{what}: CONT is needed with aerosols (phasarr given)")
        cont, ncont = self._fused_cont_args(what, n, L, q, FRAC, TOTAM, DELH, CONT, IRAY, f4, variant, ncont=npop)
        out = np.empty((n, W, P))
        head = (self._ctx, int(ISPACE), n, L, _ptr(lp), _ptr(lt), _ptr(am), *cont, ncont, nth)
        tail = (_ptr(rg), P, _ptr(sol), _ptr(emi), _ptr(aph), _ptr(_np(solar)), int(lowbc), _ptr(_np(brdf_matrix)), nmu,
                _ptr(mu1), _ptr(_np(wt1)), int(nf), int(nphi), int(iray), int(imie), _ptr(_np(xfac)), _ptr(out), *axis)
        if theta is not None:
            rc = self._lib.ansfm_cirsrad_ck_scatter_batch_src(*head, _ptr(theta), _ptr(mu_theta), *tail)
        else:
            rc = self._lib.ansfm_cirsrad_ck_scatter_batch_cont(*head, _ptr(phasarr), *tail)
        self._check(rc, what)
        return out

    def last_scatter_cache(self):
        """(layers of models 1..n-1 taken from model 0's doubling results, all such layers) of the last batched scatter call"""
        a = C.c_int64(); b = C.c_int64()
        self._check(self._lib.ansfm_last_scatter_cache(self._ctx, C.byref(a), C.byref(b)), "last_scatter_cache")
        return int(a.value), int(b.value)

    def last_scatter_windows(self):
        """(spectral windows of phase matrices / Hansen factors, wavenumbers per window) of the last scattering call: more
        than one window only at G = 1 (LBL tables) when the axis is longer than a window (ANSFM_MS_WINDOW overrides its size)"""
        a = C.c_int64(); b = C.c_int64()
        self._check(self._lib.ansfm_last_scatter_windows(self._ctx, C.byref(a), C.byref(b)), "last_scatter_windows")
        return int(a.value), int(b.value)

    def add_line_set_monochromatic_absorption(self, wn_grid, lineshape_id, t_calc, t_ref, p_calc, p_ref, q_ratio,
                                              isotopic_abundance, isotopic_mass, mol_mix_frac, broadening_params, nu, sw,
                                              e_lower, stimulated_emission_at_t_ref, out, store=None, s_floor=0.0,
                                              wn_calc_window=25.0, wn_approx_window=75.0):
        """LineData_0.add_line_set_monochromatic_absorption (:280).  Scalars t_calc/p_calc/q_ratio = the reference
        call (out (nw,), store (4,N)); 1-D arrays of length L = batched over (T,p) points (out (L,nw), store (L,4,N)).
        `out` (float64, C-contiguous) is added to in place and returned."""
        wn_grid = _np(wn_grid); mmf = _np(mol_mix_frac); bp = _np(broadening_params)
        t = _np(np.atleast_1d(t_calc)); p = _np(np.atleast_1d(p_calc)); q = _np(np.atleast_1d(q_ratio))
        L = t.shape[0]
        nu = _np(nu); N = nu.shape[0]; M = mmf.shape[0]
        if out.dtype != np.float64 or not out.flags.c_contiguous or out.size != L * wn_grid.shape[0]:
            raise ValueError("out must be a C-contiguous float64 array of shape (nw,) or (L,nw)")
        if store is not None and (store.dtype != np.float64 or not store.flags.c_contiguous or store.size != L * 4 * N):
            raise ValueError("store must be a C-contiguous float64 array of shape (4,N) or (L,4,N)")
        rc = self._lib.ansfm_add_line_set_monochromatic_absorption(
            self._ctx, wn_grid.shape[0], _ptr(wn_grid), int(lineshape_id), L, _ptr(t), float(t_ref), _ptr(p), float(p_ref),
            _ptr(q), float(isotopic_abundance), float(isotopic_mass), M, _ptr(mmf), N, _ptr(bp), _ptr(nu), _ptr(_np(sw)),
            _ptr(_np(e_lower)), _ptr(_np(stimulated_emission_at_t_ref)), _ptr(out), _ptr(store), float(s_floor),
            float(wn_calc_window), float(wn_approx_window))
        self._check(rc, "add_line_set_monochromatic_absorption")
        return out

    def add_pseudo_continuum_monochromatic_absorption(self, wn_grid, lineshape_id, t_calc, t_ref, p_calc, p_ref, q_ratio,
                                                      isotopic_abundance, isotopic_mass, mol_mix_frac,
                                                      lsw_mean_broadening_params, wn_bin_centers, wn_bin_widths, sw_sum,
                                                      lsw_mean_e_lower, out, store=None, store_x=None, n_neighbour_bins=3):
        """LineData_0.add_pseudo_continuum_monochromatic_absorption (:486): the pseudo-continuum of the weak lines.  Scalars
        t_calc/p_calc/q_ratio = the reference call (out (nw,), store (3,N), store_x (N,)); 1-D arrays of length L = batched
        over (T,p) points (out (L,nw), store (L,3,N), store_x (L,N)).  `out` (float64, C-contiguous) is added to in place
        and returned.  The lower bin edges must be ascending (ValueError otherwise); the reference's store_y / store_z
        scratch arrays are not part of the call."""
        wn_grid = _np(wn_grid)
        t = _np(np.atleast_1d(t_calc)); p = _np(np.atleast_1d(p_calc))
        L = t.shape[0]
        a = _PcArgs(L, q_ratio, mol_mix_frac, lsw_mean_broadening_params, wn_bin_centers, wn_bin_widths, sw_sum,
                     lsw_mean_e_lower, store, store_x)
        if out.dtype != np.float64 or not out.flags.c_contiguous or out.size != L * wn_grid.shape[0]:
            raise ValueError("out must be a C-contiguous float64 array of shape (nw,) or (L,nw)")
        rc = self._lib.ansfm_add_pseudo_continuum_monochromatic_absorption(
            self._ctx, wn_grid.shape[0], _ptr(wn_grid), int(lineshape_id), L, _ptr(t), float(t_ref), _ptr(p), float(p_ref),
            _ptr(a.q), float(isotopic_abundance), float(isotopic_mass), a.M, _ptr(a.mmf), a.N, _ptr(a.bp), _ptr(a.c), _ptr(a.w),
            _ptr(a.sw), _ptr(a.el), _ptr(out), _ptr(store), _ptr(store_x), int(n_neighbour_bins))
        self._check(rc, "add_pseudo_continuum_monochromatic_absorption")
        return out

    def mie_makephase(self, wavel, iscat, dsize, rs, refindx, theta, radius_block=None, return_counts=False, radius_cap=None):
        """Scatter_0.makephase (module level, :1828) for iscat 1 .. 4: Mie theory integrated over a size distribution.
        wavel (nwave,) um, dsize (3,), rs (3,) = first radius, last radius, step (rs[1] < rs[0]: open range), refindx (nwave,2),
        theta (ntheta,) within [0, 90] -> (xscat, xext, thetax, phas) as the reference returns them: cross-sections in cm2,
        thetax (nphas,) the angles out to 180 degrees, phas (nwave,nphas) before the class method divides by 4 pi; with
        return_counts the radii each wavelength integrated over as a fifth item.  radius_block (a multiple of 64 radii) and
        radius_cap (radii of an open range before "did not terminate") hold for this call; neither changes a bit of the
        result.  ValueError where the reference gives up (the text names wavelength and radius), for an angle outside
        [0, 90] and for another iscat."""
        wavel = _np(np.atleast_1d(wavel)); theta = _np(np.atleast_1d(theta))
        dsize = _np(dsize); rs = _np(rs); refindx = _np(refindx)
        nwave, ntheta = wavel.shape[0], theta.shape[0]
        if wavel.ndim != 1 or theta.ndim != 1 or dsize.shape != (3,) or rs.shape != (3,) or refindx.shape != (nwave, 2):
            raise ValueError("mie_makephase: wavel (nwave,), dsize (3,), rs (3,), refindx (nwave,2), theta (ntheta,)")
        nphas = 2 * ntheta - 1 if np.count_nonzero(theta == 90.0) == 1 else 2 * ntheta
        thetax = np.zeros(nphas)
        thetax[:ntheta] = theta
        for i in range(ntheta, nphas):
            thetax[i] = 180.0 - thetax[nphas - i - 1]
        xscat, xext, phas = np.empty(nwave), np.empty(nwave), np.empty((nwave, nphas))
        counts = np.zeros(nwave, dtype=np.int32)
        self._check(self._lib.ansfm_mie_set_radius_block(self._ctx, int(radius_block or 0)), "mie_set_radius_block")
        self._check(self._lib.ansfm_mie_set_radius_cap(self._ctx, int(radius_cap or 0)), "mie_set_radius_cap")
        rc = self._lib.ansfm_mie_makephase(self._ctx, nwave, _ptr(wavel), int(iscat), _ptr(dsize), _ptr(rs), _ptr(refindx), ntheta,
                                           _ptr(theta), _ptr(xscat), _ptr(xext), _ptr(phas), _ptr(counts))
        self._check(rc, "mie_makephase")
        return (xscat, xext, thetax, phas, counts) if return_counts else (xscat, xext, thetax, phas)

    def mie_last(self):
        """(kernel milliseconds, blocks of radii, radii of the largest block) of the last mie_makephase call"""
        ms, nb, nr = C.c_double(), C.c_int32(), C.c_int32()
        self._check(self._lib.ansfm_mie_last(self._ctx, C.byref(ms), C.byref(nb), C.byref(nr)), "mie_last")
        return ms.value, nb.value, nr.value

    HG_FIT_NPHASE_CAP = 8192               # angles of a phase function ansfm_hg_fit takes

    def hg_fit(self, theta, phase, return_counts=False):
        """Scatter_0.subfithgm (:1948): the double Henyey-Greenstein fit of phase functions.  theta (nphase,) degrees, phase
        (nfit, nphase) normalised to 4 pi -> (f, g1, g2, rms), each (nfit,); with return_counts a fifth item, int32
        (nfit, 2): the calls of mrqminl a fit took and the accepted ones.  ValueError for shapes that do not match, nphase
        outside 1 .. HG_FIT_NPHASE_CAP, and for a fit whose normal equations are singular (the text names the fit)."""
        theta = _np(np.atleast_1d(theta)); phase = _np(phase)
        if theta.ndim != 1 or phase.ndim != 2 or phase.shape[1] != theta.shape[0] or phase.shape[0] < 1:
            raise ValueError("hg_fit: theta (nphase,), phase (nfit, nphase)")
        nfit, nphase = phase.shape
        f, g1, g2, rms = np.empty(nfit), np.empty(nfit), np.empty(nfit), np.empty(nfit)
        counts = np.zeros((nfit, 2), dtype=np.int32)
        rc = self._lib.ansfm_hg_fit(self._ctx, nfit, nphase, _ptr(theta), _ptr(phase), _ptr(f), _ptr(g1), _ptr(g2), _ptr(rms),
                                    _ptr(counts))
        self._check(rc, "hg_fit")
        return (f, g1, g2, rms, counts) if return_counts else (f, g1, g2, rms)

    def hg_fit_last(self):
        """kernel milliseconds of the last hg_fit call"""
        ms = C.c_double()
        self._check(self._lib.ansfm_hg_fit_last(self._ctx, C.byref(ms)), "hg_fit_last")
        return ms.value

    def _phase_tables(self, what, imie, SWAVE, THETA_TAB, tab):
        """-> (imie, SWAVE, THETA_TAB or None, tab, NDUST, NTAB) as ansfm_calc_phase / ansfm_upload_phase take them"""
        imie = int(imie); SWAVE = _np(np.atleast_1d(SWAVE)); tab = _np(tab)
        if imie not in (0, 1, 2):
            raise ValueError(f"{what}: imie must be 0 (Henyey-Greenstein), 1 (tabulated) or 2 (Legendre)")
        if SWAVE.ndim != 1 or tab.ndim != 3 or tab.shape[0 if imie else 1] != SWAVE.shape[0] or (imie == 0 and tab.shape[0] != 3):
            raise ValueError(f"{what}: tab must be (3, NWAVE_scatter, NDUST) for imie 0, else (NWAVE_scatter, NTAB, NDUST)")
        THETA_TAB = _np(np.atleast_1d(THETA_TAB)) if imie == 1 else None
        if imie == 1 and THETA_TAB.shape != (tab.shape[1],):
            raise ValueError(f"{what}: THETA_TAB must be (NTAB,)")
        return imie, SWAVE, THETA_TAB, tab, tab.shape[2], (0 if imie == 0 else tab.shape[1])

    def calc_phase(self, imie, SWAVE, THETA_TAB, tab, theta, WAVEC):
        """Scatter_0.calc_phase (:760) on the GPU: imie 0 with tab = (F, G1, G2) stacked (3, NWAVE_scatter, NDUST), 1 with PHASE
        (NWAVE_scatter, NTHETA, NDUST) on THETA_TAB, 2 with WLPOL (NWAVE_scatter, NLPOL, NDUST); SWAVE = Scatter.WAVE; theta
        (nth,) degrees, WAVEC (W,) -> phase (W, nth, NDUST).  ValueError where the reference raises one (the range test, an
        angle outside THETA_TAB) and for tables that are not ascending."""
        imie, SWAVE, THETA_TAB, tab, nd, ntab = self._phase_tables("calc_phase", imie, SWAVE, THETA_TAB, tab)
        theta = _np(np.atleast_1d(theta)); WAVEC = _np(np.atleast_1d(WAVEC))
        out = np.empty((WAVEC.shape[0], theta.shape[0], nd))
        rc = self._lib.ansfm_calc_phase(self._ctx, imie, SWAVE.shape[0], _ptr(SWAVE), nd, ntab, _ptr(THETA_TAB), _ptr(tab),
                                        theta.shape[0], _ptr(theta), WAVEC.shape[0], _ptr(WAVEC), _ptr(out))
        self._check(rc, "calc_phase")
        return out

    def calc_phase_ray(self, theta):
        """Scatter_0.calc_phase_ray (:834): theta (nth,) degrees -> (nth,)"""
        theta = _np(np.atleast_1d(theta))
        out = np.empty(theta.shape[0])
        self._check(self._lib.ansfm_calc_phase_ray(self._ctx, theta.shape[0], _ptr(theta), _ptr(out)), "calc_phase_ray")
        return out

    def phase_last(self):
        """kernel milliseconds of the last calc_phase, calc_phase_ray or phase_from_source call"""
        ms = C.c_double()
        self._check(self._lib.ansfm_phase_last(self._ctx, C.byref(ms)), "phase_last")
        return ms.value

    def upload_phase(self, imie, SWAVE, THETA_TAB, tab):
        """Make the aerosol phase function a resident source on the uploaded table's grid, beside `upload_dust` (arguments as
        `calc_phase`).  NotImplementedError for more than 7 populations.  A new table clears the source."""
        imie, SWAVE, THETA_TAB, tab, nd, ntab = self._phase_tables("upload_phase", imie, SWAVE, THETA_TAB, tab)
        rc = self._lib.ansfm_upload_phase(self._ctx, imie, SWAVE.shape[0], _ptr(SWAVE), nd, ntab, _ptr(THETA_TAB), _ptr(tab))
        self._check(rc, "upload_phase")

    def phase_source_info(self):
        """(imie, NDUST) of the resident phase-function source; (-1, 0): none stands"""
        imie, nd = C.c_int(), C.c_int()
        self._check(self._lib.ansfm_phase_source_info(self._ctx, C.byref(imie), C.byref(nd)), "phase_source_info")
        return imie.value, nd.value

    def phase_from_source(self, theta):
        """phase (NWAVE, nth, NDUST) of the resident source on the table's grid: `calc_phase` with WAVEC = that grid, bit for bit"""
        theta = _np(np.atleast_1d(theta))
        out = np.empty((self.ktable_info()[0][0], theta.shape[0], self.phase_source_info()[1]))
        self._check(self._lib.ansfm_phase_from_source(self._ctx, theta.shape[0], _ptr(theta), _ptr(out)), "phase_from_source")
        return out

    def phasarr_from_source(self, theta):
        """the array `cirsrad_ck_scatter_batch_src` forms from the resident source at theta (Scatter.THETA, ascending):
        PHASE_ARRAY[:, :, :, ::-1] of ForwardModel_0.py:5128-5142, (NDUST, NWAVE, 2, nth)"""
        theta = _np(np.atleast_1d(theta))
        out = np.empty((self.phase_source_info()[1], self.ktable_info()[0][0], 2, theta.shape[0]))
        rc = self._lib.ansfm_phasarr_from_source(self._ctx, theta.shape[0], _ptr(theta), _ptr(_np(np.cos(theta * np.pi / 180))), _ptr(out))
        self._check(rc, "phasarr_from_source")
        return out

    SURFACE_NPAR = {1: 1, 2: 10, 3: 2}     # rows of `params` per LowerBoundaryConditionEnum value

    def _surface_params(self, what, lowbc, params, zero_ok=False):
        lowbc = int(lowbc)
        if lowbc not in self.SURFACE_NPAR and not (zero_ok and lowbc == 0):
            raise ValueError("%s: lowbc %d is not 1 LAMBERTIAN, 2 HAPKE or 3 OREN_NAYAR%s" % (what, lowbc, ", or 0" if zero_ok else ""))
        params = np.atleast_2d(_np(params))
        if params.ndim != 2 or params.shape[1] < 1 or (lowbc and params.shape[0] != self.SURFACE_NPAR[lowbc]):
            raise ValueError("%s: params must be (%s, nwave) for lowbc %d, got %s"
                             % (what, self.SURFACE_NPAR.get(lowbc, "any"), lowbc, params.shape))
        return lowbc, params

    def surface_brdf(self, lowbc, params, SOL_ANG, EMISS_ANG, AZI_ANG):
        """Surface_0.calc_BRDF (:916) after its interpolation onto the wavenumbers: params (npar, nwave) -- LOWBC 1 the albedo,
        2 the ten arguments of calc_Hapke_BRDF in its order, 3 (A, ROUGHNESS) -- at the angle triples SOL_ANG, EMISS_ANG,
        AZI_ANG (NTHETA,) in degrees -> BRDF (nwave, NTHETA)."""
        lowbc, params = self._surface_params("surface_brdf", lowbc, params)
        sol, emi, azi = (_np(np.atleast_1d(a)) for a in (SOL_ANG, EMISS_ANG, AZI_ANG))
        if sol.ndim != 1 or sol.shape[0] < 1 or emi.shape != sol.shape or azi.shape != sol.shape:
            raise ValueError("surface_brdf: SOL_ANG, EMISS_ANG and AZI_ANG must be 1-D of one length, got %s %s %s"
                             % (sol.shape, emi.shape, azi.shape))
        nwave, ntheta = params.shape[1], sol.shape[0]
        out = np.empty((nwave, ntheta))
        rc = self._lib.ansfm_surface_brdf(self._ctx, lowbc, nwave, _ptr(params), ntheta, _ptr(sol), _ptr(emi), _ptr(azi), _ptr(out))
        self._check(rc, "surface_brdf")
        return out

    @staticmethod
    def brdf_tables(MU, NPHI, NF):
        """The tables of ansfm_brdf_matrix that depend on the quadrature alone, in calc_brdf_matrix's own expressions
        (ForwardModel_0.py:5198-5245) so that they carry its bits: MU as Scatter stores it -> the angles of MU[::-1], the
        azimuths k dphi in degrees, their fold into [0, 180] (Surface_0.py:1363-1381), wphi and cos(ic k dphi)."""
        mu = np.zeros(len(MU))
        mu[:] = np.asarray(MU, dtype=_f8)[::-1]
        dphi = 2.0 * np.pi / NPHI
        k = np.arange(NPHI + 1)
        ang = np.arccos(mu) * 180.0 / np.pi
        azi = (k * dphi) * 180.0 / np.pi
        phi = 180. - azi
        phix = np.where(phi > 180., 180. - (phi - 180.), np.where(phi < 0., -phi, phi))
        wphi = np.full(NPHI + 1, (1.0 * dphi) / (2.0 * np.pi))
        wphi[0] = wphi[NPHI] = (0.5 * dphi) / (2.0 * np.pi)
        cosk = np.cos(np.arange(NF + 1)[:, None] * (k * dphi)[None, :])
        return ang, azi, phix, wphi, np.ascontiguousarray(cosk)

    def brdf_matrix(self, lowbc, params, MU, NPHI, NF):
        """ForwardModel_0.calc_brdf_matrix (:5168) after the interpolation of the surface parameters onto the wavenumbers:
        params as for surface_brdf, MU = Scatter.MU as stored (it is reversed here, as there) -> BRDF_mat (nwave, NMU, NMU,
        NF + 1).  LOWBC 2 is integrated over azimuth on the device; 1 gives albedo / pi in plane 0; 0 and 3 give zeros."""
        lowbc, params = self._surface_params("brdf_matrix", lowbc, params, zero_ok=True)
        MU = _np(np.atleast_1d(MU))
        NPHI, NF = int(NPHI), int(NF)
        if MU.ndim != 1 or MU.shape[0] < 1 or NPHI < 1 or NF < 0:
            raise ValueError("brdf_matrix: nmu >= 1, nphi >= 1 and nf >= 0 are needed, got nmu %s, nphi %d, nf %d"
                             % (MU.shape, NPHI, NF))
        ang, azi, phix, wphi, cosk = self.brdf_tables(MU, NPHI, NF)
        nwave, nmu = params.shape[1], MU.shape[0]
        out = np.empty((nwave, nmu, nmu, NF + 1))
        rc = self._lib.ansfm_brdf_matrix(self._ctx, lowbc, nwave, _ptr(params), nmu, _ptr(ang), NPHI, NF, _ptr(azi), _ptr(phix),
                                         _ptr(wphi), _ptr(cosk), _ptr(out))
        self._check(rc, "brdf_matrix")
        return out

    def brdf_last(self):
        """kernel milliseconds of the last surface_brdf / brdf_matrix call"""
        ms = C.c_double()
        self._check(self._lib.ansfm_brdf_last(self._ctx, C.byref(ms)), "brdf_last")
        return ms.value

    def lbl_accumulator(self, wn_grid, t_calc, p_calc):
        """The runtime line-by-line opacity of a gas summed in HBM: a zeroed (L, nw) accumulator on this engine's device for
        the grid and the (T,p) points given (see LblAccumulator).  The engine owns one; a new one starts over."""
        return LblAccumulator(self, wn_grid, t_calc, p_calc)

    def layer_average(self, RADIUS, H, P, T, ID, VMR, DUST, PARAH2, BASEH, BASEP=None, LAYANG=0.0, LAYINT=0, LAYHT=0.0,
                      NINT=101, DUST_UNITS=None, XMOLWT=None):
        """Layer_0.layer_average (:755), same argument order (ID and BASEP are unused there too).  A leading
        state axis on H/P/T/VMR/DUST/PARAH2/BASEH batches the call.  Returns
        HEIGHT,PRESS,TEMP,TOTAM,AMOUNT,PP,CONT,FRAC,DELH,BASET,LAYSF."""
        return self._layer_average(False, RADIUS, H, P, T, VMR, DUST, PARAH2, BASEH, LAYANG, LAYINT, LAYHT, NINT,
                                   DUST_UNITS, XMOLWT)

    def layer_averageg(self, RADIUS, H, P, T, ID, VMR, DUST, PARAH2, BASEH, BASEP=None, LAYANG=0.0, LAYINT=0, LAYHT=0.0,
                       NINT=101, DUST_UNITS=None, XMOLWT=None):
        """Layer_0.layer_averageg (:1032): layer_average's outputs followed by DTE, DAM, DCO, DPH (NLAY, NPRO)."""
        return self._layer_average(True, RADIUS, H, P, T, VMR, DUST, PARAH2, BASEH, LAYANG, LAYINT, LAYHT, NINT,
                                   DUST_UNITS, XMOLWT)

    def _layer_average(self, grad, RADIUS, H, P, T, VMR, DUST, PARAH2, BASEH, LAYANG, LAYINT, LAYHT, NINT, DUST_UNITS, XMOLWT):
        H = _np(H); single = H.ndim == 1
        H2 = np.atleast_2d(H); n, NPRO = H2.shape
        P2 = _np(P).reshape(n, NPRO); T2 = _np(T).reshape(n, NPRO)
        V2 = _np(VMR).reshape(n, NPRO, -1); NV = V2.shape[2]
        D2 = None if DUST is None else _np(DUST).reshape(n, NPRO, -1)
        ND = 0 if D2 is None else D2.shape[2]
        PH = None if PARAH2 is None else _np(PARAH2).reshape(n, NPRO)
        XM = None if XMOLWT is None else _np(np.broadcast_to(_np(XMOLWT).reshape(-1, NPRO), (n, NPRO)))
        BH = _np(np.broadcast_to(_np(BASEH).reshape(-1, np.shape(BASEH)[-1]), (n, np.shape(BASEH)[-1]))); NL = BH.shape[1]
        mk = lambda *shape: np.empty(shape)
        HEIGHT, PRESS, TEMP, TOTAM, FRAC, DELH, BASET, LAYSF = (mk(n, NL) for _ in range(8))
        AMOUNT, PPo, CONT = mk(n, NL, NV), mk(n, NL, NV), mk(n, NL, ND)
        args = [self._ctx, n, float(RADIUS), NPRO, _ptr(H2), _ptr(P2), _ptr(T2), NV, _ptr(V2), ND, _ptr(D2), _ptr(PH), NL, _ptr(BH),
                float(LAYANG), int(LAYINT), float(LAYHT), int(NINT), _ptr(_np(DUST_UNITS, np.int32)), _ptr(XM), _ptr(HEIGHT),
                _ptr(PRESS), _ptr(TEMP), _ptr(TOTAM), _ptr(AMOUNT), _ptr(PPo), _ptr(CONT), _ptr(FRAC), _ptr(DELH), _ptr(BASET),
                _ptr(LAYSF)]
        out = (HEIGHT, PRESS, TEMP, TOTAM, AMOUNT, PPo, CONT, FRAC, DELH, BASET, LAYSF)
        if grad:
            M = tuple(mk(n, NL, NPRO) for _ in range(4))
            self._check(self._lib.ansfm_layer_averageg(*args, *(_ptr(m) for m in M)), "layer_averageg")
            out = out + M
        else:
            self._check(self._lib.ansfm_layer_average(*args), "layer_average")
        return tuple(a[0] for a in out) if single else out

    def layer_average_dev(self, RADIUS, H, P, T, VMR, DUST, PARAH2, BASEH, LAYANG=0.0, LAYINT=0, LAYHT=0.0, NINT=101,
                          DUST_UNITS=None, XMOLWT=None):
        """Layer_0.layer_average for n states whose profiles are torch device tensors -- H, P, T (n, NPRO), VMR (n, NPRO,
        NVMR), DUST (n, NPRO, NDUST) / PARAH2 / XMOLWT (n, NPRO) or None, BASEH (n, NLAY), all float64 and contiguous --
        with the layers left in HBM: dict of device tensors HEIGHT .. LAYSF (n, NLAY), AMOUNT, PP (n, NLAY, NVMR), CONT
        (n, NLAY, NDUST), views of one buffer.  Asynchronous on the engine's stream."""
        import torch
        n, NPRO = H.shape
        NV = VMR.shape[2]; NL = BASEH.shape[1]
        ND = 0 if DUST is None else DUST.shape[2]
        for a in (H, P, T, VMR, DUST, PARAH2, XMOLWT, BASEH):
            if a is not None and (a.dtype != torch.float64 or not a.is_contiguous() or not a.is_cuda or a.shape[0] != n):
                raise ValueError("layer_average_dev: contiguous float64 device tensors with the state axis first")
        nl = n * NL
        buf = torch.empty(nl * (8 + 2 * NV + ND), dtype=torch.float64, device=H.device)
        rc = self._lib.ansfm_layer_average_dev(self._ctx, n, float(RADIUS), NPRO, _ptr(H), _ptr(P), _ptr(T), NV, _ptr(VMR), ND,
                                               _ptr(DUST), _ptr(PARAH2), NL, _ptr(BASEH), float(LAYANG), int(LAYINT), float(LAYHT),
                                               int(NINT), _ptr(_np(DUST_UNITS, np.int32)), _ptr(XMOLWT), _ptr(buf))
        self._check(rc, "layer_average_dev")
        out = {name: buf[k * nl:(k + 1) * nl].view(n, NL)
               for k, name in enumerate(("HEIGHT", "PRESS", "TEMP", "TOTAM", "FRAC", "DELH", "BASET", "LAYSF"))}
        o = 8 * nl
        out["AMOUNT"] = buf[o:o + nl * NV].view(n, NL, NV); o += nl * NV
        out["PP"] = buf[o:o + nl * NV].view(n, NL, NV); o += nl * NV
        out["CONT"] = buf[o:o + nl * ND].view(n, NL, ND)
        return out

    def map2pro(self, dSPECIN, NWAVE, NVMR, NDUST, NPRO, NPATH, NLAYIN, LAYINC, DTE, DAM, DCO, INCPAR=(-1,), to_host=True):
        """ForwardModel_0.map2pro (:5319), same arguments -> dSPECOUT (NWAVE, NVMR+2+NDUST, NPRO, NPATH).
        When dSPECIN is the very array the last cirsradg_ck_thermal call returned, its device copy is used
        (no host->device transfer); the result stays on the device for a following map2xvec.  dSPECIN = None: the
        gradients a `cirsradg_ck_thermal(..., gradients_on_device=True)` call left on the device.  to_host = False: the
        result is not copied back either (None is returned; `map2xvec(None, ...)` continues from the device)."""
        dev_in = dSPECIN is None
        if dev_in:
            ch = getattr(self, "_chain_dspec", None)
            if not (isinstance(ch, tuple) and ch[0] == "device"):
                raise ValueError("map2pro: no device-resident cirsradg result (gradients_on_device=True) to continue from")
            W, NPAR, LIMAX, P = ch[1:]
        else:
            dSPECIN = _np(dSPECIN)
            W, NPAR, LIMAX, P = dSPECIN.shape
        if W != NWAVE or NPAR != NVMR + 2 + NDUST or P != NPATH:
            raise ValueError("map2pro: dSPECIN must be (NWAVE, NVMR+2+NDUST, NLAYIN, NPATH)")
        LAYINC = _np(LAYINC, np.int32)
        if LAYINC.ndim == 1:
            LAYINC = LAYINC[:, None]
        if LAYINC.shape != (LIMAX, P):
            raise ValueError("shapes (%d,%d) and %s not aligned: LAYINC rows must equal dSPECIN's layer axis"
                             % (W, LIMAX, LAYINC.shape))
        DTE = _np(DTE); DAM = _np(DAM); DCO = _np(DCO)
        NLAY = DTE.shape[0]
        inc = None if INCPAR[0] == -1 else _np(list(INCPAR), np.int32)
        if inc is not None and inc[0] > NVMR + NDUST:
            raise UnboundLocalError("local variable 'dSPECOUT1' referenced before assignment")   # as the reference
        out = np.empty((W, NPAR, NPRO, P)) if to_host else None
        chained = dev_in or (getattr(self, "_chain_dspec", None) is not None and self._chain_dspec == _fingerprint(dSPECIN))
        rc = self._lib.ansfm_map2pro(self._ctx, W, NPAR, LIMAX, P, int(NPRO), NLAY, int(NVMR), int(NDUST),
                                     None if chained else _ptr(dSPECIN), _ptr(LAYINC), _ptr(DTE), _ptr(DAM), _ptr(DCO),
                                     0 if inc is None else len(inc), _ptr(inc), _ptr(out))
        self._check(rc, "map2pro")
        if out is None:
            self._chain_map = ("device", W, NPAR, int(NPRO), P)
            return None
        out.flags.writeable = False      # its device twin feeds map2xvec
        self._chain_map = _fingerprint(out)
        return out

    def map2xvec(self, dSPECIN, NWAVE, NVMR, NDUST, NPRO, NPATH, NX, xmap):
        """ForwardModel_0.map2xvec (:5387), same arguments -> dSPECOUT (NWAVE, NPATH, NX).  dSPECIN = None: the result a
        `map2pro(..., to_host=False)` call left on the device."""
        if dSPECIN is None:
            ch = getattr(self, "_chain_map", None)
            if not (isinstance(ch, tuple) and ch[0] == "device"):
                raise ValueError("map2xvec: no device-resident map2pro result (to_host=False) to continue from")
            W, NPAR, NPROi, P = ch[1:]
        else:
            dSPECIN = _np(dSPECIN)
            W, NPAR, NPROi, P = dSPECIN.shape
        xmap = _np(xmap)
        if xmap.shape != (NX, NPAR, NPROi):
            raise ValueError("shape-mismatch for sum")     # np.tensordot's message
        out = np.empty((W, P, NX))
        chained = dSPECIN is None or (getattr(self, "_chain_map", None) is not None and self._chain_map == _fingerprint(dSPECIN))
        rc = self._lib.ansfm_map2xvec(self._ctx, W, NPAR, NPROi, P, int(NX), None if chained else _ptr(dSPECIN),
                                      _ptr(xmap), _ptr(out))
        self._check(rc, "map2xvec")
        return out

    # ---- continuum -----------------------------------------------------------------------------------------------
    def calc_tau_cia(self, ISPACE, WAVEC, CIA_WAVEN, CIA_TEMP, CIA_FRAC, NPARA, K_CIA, IPAIRG1, IPAIRG2, INORMALT, INORMAL,
                     INORMALD, ID, ISO, PP, PRESS, TEMP, FRAC, TOTAM, DELH, k_co2=None, k_n2n2=None, k_n2h2=None, with_grad=True):
        """ForwardModel_0.calc_tau_cia (:4516) with the reference's objects flattened into arrays (CIA.WAVEN/TEMP/FRAC/
        NPARA/K_CIA/IPAIRG1/IPAIRG2/INORMALT/INORMAL, CIA.locate_INORMAL_pairs(), Atmosphere.ID/ISO, Layer.PP/PRESS/TEMP/
        FRAC/TOTAM/DELH) and co2cia / n2n2cia / n2h2cia(WAVEN) as vectors.  -> TAUCIA (NWAVE,NLAY), dTAUCIA (NWAVE,NLAY,NVMR+2)."""
        WAVEC = _np(WAVEC); ID = np.asarray(ID); ISO = np.asarray(ISO)
        NVMR = ID.size
        if int(ISPACE) == 0:
            WAVEN, isort = WAVEC, None
        else:                                              # :4565-4568
            WAVEN = 1.e4 / WAVEC; isort = np.argsort(WAVEN); WAVEN = _np(WAVEN[isort])
        K = _np(K_CIA); NPAIR, NPE, NT, NWC = K.shape
        g1, g2, ico2, in2, ih2 = self._cia_gases(NPAIR, IPAIRG1, IPAIRG2, INORMALT, INORMAL, INORMALD, ID, ISO)
        q = _np((_np(PP).T / _np(PRESS)).T)
        L = q.shape[0]
        xfac = _np((_np(TOTAM) * 1.0e-4) ** 2. / (_np(DELH) * 1.0e2))
        frac = _np(np.asarray(CIA_FRAC, float).reshape(-1))
        W = WAVEN.size
        tau = np.empty((W, L)); dtau = np.empty((W, L, NVMR + 2)) if with_grad else None
        rc = self._lib.ansfm_calc_tau_cia(self._ctx, W, _ptr(WAVEN), NWC, _ptr(_np(CIA_WAVEN)), NPAIR, NPE, NT, _ptr(K),
                                          _ptr(_np(CIA_TEMP)), frac.size, _ptr(frac), int(NPARA), _ptr(g1), _ptr(g2), L, NVMR,
                                          _ptr(_np(TEMP)), _ptr(_np(FRAC)), _ptr(q), _ptr(xfac), ico2, _ptr(_np(k_co2)), in2,
                                          _ptr(_np(k_n2n2)), ih2, _ptr(_np(k_n2h2)), _ptr(tau), _ptr(dtau))
        self._check(rc, "calc_tau_cia")
        if isort is not None:                              # :4741-4743
            tau = tau[isort, :]
            dtau = None if dtau is None else dtau[isort, :, :]
        return (tau, dtau) if with_grad else tau

    @staticmethod
    def _cia_gases(NPAIR, IPAIRG1, IPAIRG2, INORMALT, INORMAL, INORMALD, ID, ISO):
        """What calc_tau_cia resolves on the host before any layer: the atmospheric gas of each partner of every pair (-1:
        pair not used) and the indices of CO2, N2 and H2 (-1: absent)."""
        g1 = np.full(NPAIR, -1, np.int32); g2 = np.full(NPAIR, -1, np.int32)
        for ip in range(NPAIR):                            # :4676-4701
            a = np.where(ID == int(IPAIRG1[ip]))[0]; b = np.where(ID == int(IPAIRG2[ip]))[0]
            if len(a) > 1: a = np.where((ID == int(IPAIRG1[ip])) & (ISO == 1))[0]
            if len(b) > 1: b = np.where((ID == int(IPAIRG2[ip])) & (ISO == 1))[0]
            if len(a) == 1 and len(b) == 1 and not (INORMALD[ip] and int(INORMALT[ip]) != int(INORMAL)):
                g1[ip], g2[ip] = a[0], b[0]
        ico2 = ih2 = in2 = -1                              # :4545-4561
        for i in range(ID.size):
            if ID[i] == 39 and ISO[i] in (0, 1): ih2 = i
            if ID[i] == 22: in2 = i
            if ID[i] == 2 and ISO[i] in (0, 1): ico2 = i
        return g1, g2, ico2, in2, ih2

    def upload_cia(self, ISPACE, WAVEC, CIA_WAVEN, CIA_TEMP, CIA_FRAC, NPARA, K_CIA, IPAIRG1, IPAIRG2, INORMALT, INORMAL,
                   INORMALD, ID, ISO, k_co2=None, k_n2n2=None, k_n2h2=None):
        """Make the CIA table a resident opacity source of the context, on the uploaded table's grid, for
        cirsrad_ck_thermal_cont_dev: the arguments of calc_tau_cia up to ISO (WAVEC: None or the table's grid, checked) and
        co2cia / n2n2cia / n2h2cia at x = WAVE (ISPACE 0) or 1e4 / WAVE (ISPACE 1), in the order of the table's grid.
        NotImplementedError for a para-H2 table whose bracket could leave K_CIA (NPARA > 0 without NPARA == len(FRAC) ==
        K_CIA.shape[1] >= 2).  A new table clears the source."""
        ID = np.asarray(ID); ISO = np.asarray(ISO)
        if WAVEC is not None:
            (W, G, NP, NT, _), _ = self.ktable_info()
            WAVE = np.empty(W)
            self._check(self._lib.ansfm_ktable_grids(self._ctx, _ptr(WAVE), _ptr(np.empty(NP)), _ptr(np.empty(NT)), _ptr(np.empty(G))),
                        "ktable_grids")
            if not np.array_equal(_np(WAVEC).reshape(-1), WAVE):
                raise ValueError("upload_cia: WAVEC is not the grid of the uploaded table")
        K = _np(K_CIA); NPAIR, NPE, NT, NWC = K.shape
        g1, g2, ico2, in2, ih2 = self._cia_gases(NPAIR, IPAIRG1, IPAIRG2, INORMALT, INORMAL, INORMALD, ID, ISO)
        frac = _np(np.asarray(CIA_FRAC, float).reshape(-1))
        rc = self._lib.ansfm_upload_cia(self._ctx, int(ISPACE), NWC, _ptr(_np(CIA_WAVEN)), NPAIR, NPE, NT, _ptr(K), _ptr(_np(CIA_TEMP)),
                                        frac.size, _ptr(frac), int(NPARA), _ptr(g1), _ptr(g2), ID.size, ico2, _ptr(_np(k_co2)), in2,
                                        _ptr(_np(k_n2n2)), ih2, _ptr(_np(k_n2h2)))
        self._check(rc, "upload_cia")
        self.cia_nvmr = int(ID.size)

    def upload_dust(self, SWAVE, KEXT, KSCA=None):
        """Make the aerosol extinction a resident opacity source of the context: KEXT (NWAVE_scatter, NDUST) on SWAVE is
        evaluated on the uploaded table's grid as calc_tau_dust evaluates it (KSCA decides with KEXT where the linear
        interpolant replaces the spline; None: zeros).  NotImplementedError for more than 7 populations.  A new table clears
        the source."""
        SWAVE = _np(SWAVE); KEXT = _np(KEXT); KSCA = _np(KSCA)
        if KEXT.ndim != 2 or KEXT.shape[0] != SWAVE.size or (KSCA is not None and KSCA.shape != KEXT.shape):
            raise ValueError("KEXT / KSCA must be (len(Scatter.WAVE), NDUST)")
        rc = self._lib.ansfm_upload_dust(self._ctx, SWAVE.size, _ptr(SWAVE), KEXT.shape[1], _ptr(KEXT), _ptr(KSCA))
        self._check(rc, "upload_dust")
        self.dust_n = int(KEXT.shape[1])

    def clear_continuum_sources(self):
        self._check(self._lib.ansfm_clear_continuum_sources(self._ctx), "clear_continuum_sources")

    def calc_tau_rayleigh(self, IRAY, ISPACE, WAVEC, TOTAM, ID=None, ISO=None, VMR=None, variant=None):
        """ForwardModel_0.calc_tau_rayleigh (:4869): IRAY 0 -> zeros, 1 -> calc_tau_rayleighj, 2 -> calc_tau_rayleighv2,
        4 -> calc_tau_rayleighls (needs ID, ISO, VMR (NLAY, NVMR)); variant='v' -> calc_tau_rayleighv (:5598).
        -> TAURAY (NWAVE, NLAY), dTAURAY (NWAVE, NLAY)."""
        WAVEC = _np(WAVEC); TOTAM = _np(TOTAM)
        W, L = WAVEC.size, TOTAM.size
        IRAY = int(IRAY)
        if variant is None and IRAY == 0:
            return np.zeros((W, L)), np.zeros((W, L))
        mode = 12 if variant == "v" else IRAY
        if mode not in (1, 2, 4, 12):
            raise ValueError("error in CIRSrad :: IRAY = " + str(IRAY) + " type has not been implemented yet")
        f4 = None
        if mode == 4:
            ID = np.asarray(ID); ISO = np.asarray(ISO); VMR = _np(VMR)
            f4 = np.zeros((L, 4))
            for j in range(ID.size):                               # :5748-5767 (the last matching gas wins)
                if ISO[j] in (0, 1):
                    col = {39: 0, 40: 1, 6: 2, 11: 3}.get(int(ID[j]))
                    if col is not None:
                        f4[:, col] = VMR[:, j]
            f4 = _np(f4)
        tau = np.empty((W, L)); dtau = np.empty((W, L))
        rc = self._lib.ansfm_calc_tau_rayleigh(self._ctx, mode, int(ISPACE), W, _ptr(WAVEC), L, _ptr(TOTAM), _ptr(f4), _ptr(tau),
                                               _ptr(dtau))
        self._check(rc, "calc_tau_rayleigh")
        return tau, dtau

    def calc_tau_rayleigh_batch_dev(self, IRAY, ISPACE, TOTAM, out, ID=None, ISO=None, VMR=None, variant=None):
        """calc_tau_rayleigh (:4869) for the n states of a batch on the uploaded table's wavenumber grid, left in HBM:
        TOTAM (n, NLAY) host, VMR (n, NLAY, NVMR) host for IRAY 4, out = torch device tensor (n, NWAVE, NLAY) float64."""
        mode = 12 if variant == "v" else int(IRAY)
        if mode not in (1, 2, 4, 12):
            raise ValueError("error in CIRSrad :: IRAY = " + str(IRAY) + " type has not been implemented yet")
        if not isinstance(TOTAM, np.ndarray) and hasattr(TOTAM, "data_ptr"):      # torch device tensors (layer_average_dev)
            import torch
            n, L = TOTAM.shape
            f4 = self.rayleigh_f4(ID, ISO, VMR) if mode == 4 else None
            if tuple(out.shape)[0] != n or tuple(out.shape)[2] != L or not out.is_contiguous() or not TOTAM.is_contiguous():
                raise ValueError("out must be a contiguous (n, NWAVE, NLAY) float64 device tensor")
            rc = self._lib.ansfm_calc_tau_rayleigh_batch_dev_in(self._ctx, mode, int(ISPACE), n, L, _ptr(TOTAM), _ptr(f4), _ptr(out))
            self._check(rc, "calc_tau_rayleigh_batch_dev")
            self._keep = (TOTAM, f4)          # alive until the next call: the kernel may still be queued
            return out
        TOTAM = _np(TOTAM)
        n, L = TOTAM.shape
        f4 = None
        if mode == 4:
            ID = np.asarray(ID); ISO = np.asarray(ISO); VMR = _np(VMR).reshape(n, L, -1)
            f4 = np.zeros((n, L, 4))
            for j in range(ID.size):                               # :5748-5767 (the last matching gas wins)
                if ISO[j] in (0, 1):
                    col = {39: 0, 40: 1, 6: 2, 11: 3}.get(int(ID[j]))
                    if col is not None:
                        f4[:, :, col] = VMR[:, :, j]
            f4 = _np(f4)
        if tuple(out.shape)[0] != n or tuple(out.shape)[2] != L or not out.is_contiguous():
            raise ValueError("out must be a contiguous (n, NWAVE, NLAY) float64 device tensor")
        rc = self._lib.ansfm_calc_tau_rayleigh_batch_dev(self._ctx, mode, int(ISPACE), n, L, _ptr(TOTAM), _ptr(f4), _ptr(out))
        self._check(rc, "calc_tau_rayleigh_batch_dev")
        return out

    def calc_tau_dust(self, WAVEC, SWAVE, KEXT, KSCA, CONT):
        """ForwardModel_0.calc_tau_dust (:4790): KEXT / KSCA (NWAVE_scatter, NDUST) on SWAVE, CONT (NLAY, NDUST) ->
        TAUDUST, TAUCLSCAT, dTAUDUSTdq, dTAUCLSCATdq (NWAVE, NLAY, NDUST)."""
        WAVEC = _np(WAVEC); SWAVE = _np(SWAVE); KEXT = _np(KEXT); KSCA = _np(KSCA); CONT = _np(CONT)
        W, L, ND = WAVEC.size, CONT.shape[0], CONT.shape[1]
        if KEXT.shape != (SWAVE.size, ND) or KSCA.shape != KEXT.shape:
            raise ValueError("KEXT / KSCA must be (len(Scatter.WAVE), NDUST)")
        out = [np.empty((W, L, ND)) for _ in range(4)]
        if ND == 0:
            return tuple(out)
        rc = self._lib.ansfm_calc_tau_dust(self._ctx, W, _ptr(WAVEC), SWAVE.size, _ptr(SWAVE), ND, _ptr(KEXT), _ptr(KSCA), L,
                                           _ptr(CONT), *[_ptr(o) for o in out])
        self._check(rc, "calc_tau_dust")
        return tuple(out)

    def kdist_bins(self, wavecalc, kabs, vbinmin, vbinmax, g_ord, fil=None):
        """Numerical core of Spectroscopy_0.calc_ktable_chunk (:3620-3652): k-distribution of the line-by-line spectrum
        kabs on the uniform grid wavecalc inside each bin [vbinmin, vbinmax], read at the g-ordinates.  fil = (bin
        centres, nfil (nbin), dfil (NF, nbin) = VFIL - VCONV, afil (NF, nbin)) weights the points with the instrument
        function, None = equal weights.  -> (nbin, NG)."""
        wavecalc = _np(wavecalc); kabs = _np(kabs); vbinmin = _np(vbinmin); vbinmax = _np(vbinmax); g_ord = _np(g_ord)
        nbin, NG = vbinmin.size, g_ord.size
        out = np.empty((nbin, NG))
        if fil is None:
            args = (None, 0, None, None, None)
        else:
            wcen, nfil, dfil, afil = _np(fil[0]), _np(fil[1], np.int32), _np(fil[2]), _np(fil[3])
            if dfil.shape != afil.shape or dfil.shape[1] != nbin or nfil.shape != (nbin,) or wcen.shape != (nbin,):
                raise ValueError("fil = (centres (nbin), nfil (nbin), dfil (NF, nbin), afil (NF, nbin))")
            args = (_ptr(wcen), dfil.shape[0], _ptr(nfil), _ptr(dfil), _ptr(afil))
        rc = self._lib.ansfm_kdist_bins(self._ctx, wavecalc.size, _ptr(wavecalc), _ptr(kabs), nbin, _ptr(vbinmin), _ptr(vbinmax),
                                        *args, NG, _ptr(g_ord), _ptr(out))
        self._check(rc, "kdist_bins")
        return out

    # ---- instrument line shape ---------------------------------------------------------------------------------
    def lblconv(self, nwave, vwave, y, nconv, vconv, ishape, fwhm):
        """Measurement_0.lblconv (:3335), one geometry: y (nwave) -> yout (nconv)."""
        return self._lblconv(vwave, y, None, nconv, vconv, ishape, fwhm)[0]

    def lblconvg(self, nwave, vwave, y, dydx, nconv, vconv, ishape, fwhm):
        """Measurement_0.lblconvg (:3799), one geometry: -> yout (nconv), gradout (nconv, nx)."""
        return self._lblconv(vwave, y, dydx, nconv, vconv, ishape, fwhm)

    def lblconv_fil(self, nwave, vwave, y, nconv, vconv, nfil, vfil, afil):
        """Measurement_0.lblconv_fil (:3549)."""
        return self._lblconv(vwave, y, None, nconv, vconv, None, None, (nfil, vfil, afil))[0]

    def lblconvg_fil(self, nwave, vwave, y, dydx, nconv, vconv, nfil, vfil, afil):
        """Measurement_0.lblconvg_fil (:3992)."""
        return self._lblconv(vwave, y, dydx, nconv, vconv, None, None, (nfil, vfil, afil))

    def lblconv_ngeom(self, nwave, vwave, y, nconv, vconv, ishape, fwhm):
        """Measurement_0.lblconv_ngeom (:3444): y (nwave, ngeom) -> yout (nconv, ngeom)."""
        return self._lblconv(vwave, y, None, nconv, vconv, ishape, fwhm, ngeom=True)[0]

    def lblconvg_ngeom(self, nwave, vwave, y, dydx, nconv, vconv, ishape, fwhm):
        """Measurement_0.lblconvg_ngeom (:3685): -> yout (nconv, ngeom), gradout (nconv, ngeom, nx)."""
        return self._lblconv(vwave, y, dydx, nconv, vconv, ishape, fwhm, ngeom=True)

    def lblconv_fil_ngeom(self, nwave, vwave, y, nconv, vconv, nfil, vfil, afil):
        """Measurement_0.lblconv_fil_ngeom (:3614)."""
        return self._lblconv(vwave, y, None, nconv, vconv, None, None, (nfil, vfil, afil), ngeom=True)[0]

    def lblconvg_fil_ngeom(self, nwave, vwave, y, dydx, nconv, vconv, nfil, vfil, afil):
        """Measurement_0.lblconvg_fil_ngeom (:3912)."""
        return self._lblconv(vwave, y, dydx, nconv, vconv, None, None, (nfil, vfil, afil), ngeom=True)

    def conv_fil(self, vwave, y, dydx, nconv, vconv, nfil, vfil, afil):
        """FWHM < 0 branch of Measurement_0.conv (:2425-2461; dydx None) / convg (:2655-2691): filter average over the
        window bracketing each filter -> yout (nconv) [, gradout (nconv, nx)]."""
        r = self._lblconv(vwave, y, dydx, nconv, vconv, None, None, (nfil, vfil, afil), bracket=True)
        return r if dydx is not None else r[0]

    def integrate_filter(self, nwave, vwave, y, nconv, vconv, nfil, vfil, afil, dydx=None):
        """Measurement_0.integrate_filter (:4079) / integrate_filterg (:4188; dydx given) and, for y (nwave, ngeom) [dydx
        (nwave, ngeom, nx)], integrate_filter_ngeom (:4131) / integrate_filterg_ngeom (:4251)."""
        r = self._lblconv(vwave, y, dydx, nconv, vconv, None, None, (nfil, vfil, afil), ngeom=(np.ndim(y) == 2), integrate=True)
        return r if dydx is not None else r[0]

    def _lblconv(self, vwave, y, dydx, nconv, vconv, ishape, fwhm, fil=None, ngeom=False, bracket=False, integrate=False):
        vwave = _np(vwave); y = _np(y); vconv = _np(np.asarray(vconv)[:nconv])
        nd = 2 if ngeom else 1
        if y.ndim != nd or (dydx is not None and np.ndim(dydx) != nd + 1):
            raise ValueError("y (nwave) and dydx (nwave, nx), or the *_ngeom shapes y (nwave, ngeom), dydx (nwave, ngeom, nx)")
        dydx = None if dydx is None else _np(dydx)
        nx = 0 if dydx is None else dydx.shape[-1]
        ng = y.shape[1] if ngeom else 1
        if dydx is not None and ngeom and dydx.shape[1] != ng:
            raise ValueError("dydx (nwave, ngeom, nx) must have the NGEOM of y")
        yout = np.empty((nconv, ng)); gout = np.empty((nconv, ng, nx))
        if fil is not None:
            nfil = _np(np.asarray(fil[0])[:nconv], np.int32)
            vfil = _np(np.asarray(fil[1])[:, :nconv]); afil = _np(np.asarray(fil[2])[:, :nconv])
        if integrate:
            rc = self._lib.ansfm_integrate_filter(self._ctx, vwave.size, _ptr(vwave), ng, _ptr(y), nx, _ptr(dydx), int(nconv),
                                                  _ptr(vconv), vfil.shape[0], _ptr(nfil), _ptr(vfil), _ptr(afil), _ptr(yout),
                                                  _ptr(gout))
            self._check(rc, "integrate_filter")
            return (yout, gout) if ngeom else (yout[:, 0], gout[:, 0, :])
        if ngeom:
            if fil is None:
                rc = self._lib.ansfm_lblconv_ngeom(self._ctx, vwave.size, _ptr(vwave), ng, _ptr(y), nx, _ptr(dydx), int(nconv),
                                                   _ptr(vconv), int(ishape), float(fwhm), _ptr(yout), _ptr(gout))
            else:
                rc = self._lib.ansfm_lblconv_fil_ngeom(self._ctx, vwave.size, _ptr(vwave), ng, _ptr(y), nx, _ptr(dydx),
                                                       int(nconv), _ptr(vconv), vfil.shape[0], _ptr(nfil), _ptr(vfil),
                                                       _ptr(afil), _ptr(yout), _ptr(gout))
            self._check(rc, "lblconv_ngeom")
            return yout, gout
        if fil is None:
            rc = self._lib.ansfm_lblconv(self._ctx, vwave.size, _ptr(vwave), _ptr(y), nx, _ptr(dydx), int(nconv), _ptr(vconv),
                                         int(ishape), float(fwhm), _ptr(yout), _ptr(gout))
        else:
            fn = self._lib.ansfm_conv_fil if bracket else self._lib.ansfm_lblconv_fil
            rc = fn(self._ctx, vwave.size, _ptr(vwave), _ptr(y), nx, _ptr(dydx), int(nconv), _ptr(vconv),
                    vfil.shape[0], _ptr(nfil), _ptr(vfil), _ptr(afil), _ptr(yout), _ptr(gout))
        self._check(rc, "lblconv")
        return yout[:, 0], gout[:, 0, :]

    def get_taugas(self, L, model=0):
        W, G = self.dims[0], self.dims[1]
        out = np.empty((W, G, L))
        self._check(self._lib.ansfm_get_taugas(self._ctx, int(model), _ptr(out)), "get_taugas")
        return out

    def get_dtaugas(self, L, model=0):
        """Side product of the last gradient CIRSrad call: (NWAVE, NG, NGAS + 1, L) -- slot s = the cross-section of gas s (times
        1e-4: the reference's dTAUGAS of that gas), slot NGAS = d tau / dT."""
        W, G, S = self.dims[0], self.dims[1], self.dims[4]
        out = np.empty((W, G, S + 1, L))
        self._check(self._lib.ansfm_get_dtaugas(self._ctx, int(model), _ptr(out)), "get_dtaugas")
        return out

    def set_layer_dedup(self, enable=True):
        """Share the gas opacity of layers that are bit-identical to the first model's inside a batched call."""
        self._check(self._lib.ansfm_set_layer_dedup(self._ctx, int(bool(enable))), "set_layer_dedup")

    def set_merge_keys(self, bits=64):
        """Row-head keys of the forward k_overlap merge: 32 (float32 keys + exact tie branch) or 64 (double keys)."""
        self._check(self._lib.ansfm_set_merge_keys(self._ctx, int(bits)), "set_merge_keys")

    def merge_redo_count(self):
        """(wave, gas) merges the 32-bit-key kernel had to rerun in its exact mode since the last table upload."""
        n = C.c_int64(0)
        self._check(self._lib.ansfm_merge_redo_count(self._ctx, C.byref(n)), "merge_redo_count")
        return int(n.value)

    def last_rt_shared(self):
        """True when the last thermal-emission or single-scattering batch started its states' paths from state 0's records (ansfm_last_rt_shared)."""
        v = C.c_int(0)
        self._check(self._lib.ansfm_last_rt_shared(self._ctx, C.byref(v)), "last_rt_shared")
        return bool(v.value)

    def last_layer_rows(self):
        """(layer opacities computed, n_models * L) of the last cirsrad_ck_thermal call."""
        a = C.c_int(); b = C.c_int()
        self._check(self._lib.ansfm_last_layer_rows(self._ctx, C.byref(a), C.byref(b)), "last_layer_rows")
        return a.value, b.value

    def last_kernel_ms(self):
        a = C.c_double(); b = C.c_double(); na = C.c_int(); nb = C.c_int()
        self._check(self._lib.ansfm_last_kernel_ms(self._ctx, C.byref(a), C.byref(na), C.byref(b), C.byref(nb)),
                    "last_kernel_ms")
        return {"overlap_ms": a.value, "overlap_launches": na.value, "rt_ms": b.value, "rt_launches": nb.value}


class _DeviceArray:
    """a device buffer described by the CUDA array interface, so that torch.as_tensor views it without a copy"""

    def __init__(self, ptr, shape, owner):
        self._owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (int(ptr), False), "version": 2,
                                         "strides": None}


class LblAccumulator:
    """The runtime line-by-line opacity of a gas, summed over its isotopologues in HBM (ansfm_lbl_accum_*): the grid and the
    (T,p) points go up once, every add leaves its term on the device, and the (L, nw) sum comes back once -- `numpy()` -- or
    stays there -- `torch()`.  The adds run the kernels of AnsfmEngine.add_line_set_monochromatic_absorption and
    add_pseudo_continuum_monochromatic_absorption and take their arguments without wn_grid, t_calc, p_calc and out: the
    sum equals the same calls on a zeroed host `out`, bit for bit.  The buffer belongs to the engine's context; the engine's
    next accumulator starts over in it, and this object then raises ValueError."""

    def __init__(self, eng, wn_grid, t_calc, p_calc):
        self._eng = eng
        wn_grid = _np(wn_grid); t = _np(np.atleast_1d(t_calc)); p = _np(np.atleast_1d(p_calc))
        if t.shape != p.shape or t.ndim != 1:
            raise ValueError("t_calc and p_calc must be 1-D arrays of one length")
        self.L, self.nw = t.shape[0], wn_grid.shape[0]
        eng._check(eng._lib.ansfm_lbl_accum_begin(eng._ctx, self.nw, _ptr(wn_grid), self.L, _ptr(t), _ptr(p)), "lbl_accum_begin")
        eng._lbl_accumulator = self

    def _live(self):
        if getattr(self._eng, "_lbl_accumulator", None) is not self:
            raise ValueError("this accumulator was replaced by a newer one of the same engine")

    def add_lines(self, lineshape_id, t_ref, p_ref, q_ratio, isotopic_abundance, isotopic_mass, mol_mix_frac,
                  broadening_params, nu, sw, e_lower, stimulated_emission_at_t_ref, store=None, s_floor=0.0,
                  wn_calc_window=25.0, wn_approx_window=75.0):
        self._live()
        eng = self._eng
        q = _np(np.atleast_1d(q_ratio)); mmf = _np(mol_mix_frac); nu = _np(nu)
        N, M = nu.shape[0], mmf.shape[0]
        if q.shape != (self.L,):
            raise ValueError("q_ratio must have one value per (T,p) point")
        if store is not None and (store.dtype != np.float64 or not store.flags.c_contiguous or store.size != self.L * 4 * N):
            raise ValueError("store must be a C-contiguous float64 array of shape (L,4,N)")
        rc = eng._lib.ansfm_lbl_accum_add_lines(
            eng._ctx, int(lineshape_id), float(t_ref), float(p_ref), _ptr(q), float(isotopic_abundance), float(isotopic_mass), M,
            _ptr(mmf), N, _ptr(_np(broadening_params)), _ptr(nu), _ptr(_np(sw)), _ptr(_np(e_lower)),
            _ptr(_np(stimulated_emission_at_t_ref)), _ptr(store), float(s_floor), float(wn_calc_window), float(wn_approx_window))
        eng._check(rc, "lbl_accum_add_lines")
        return self

    def add_pseudo_continuum(self, lineshape_id, t_ref, p_ref, q_ratio, isotopic_abundance, isotopic_mass, mol_mix_frac,
                             lsw_mean_broadening_params, wn_bin_centers, wn_bin_widths, sw_sum, lsw_mean_e_lower, store=None,
                             store_x=None, n_neighbour_bins=3):
        self._live()
        eng = self._eng
        a = _PcArgs(self.L, q_ratio, mol_mix_frac, lsw_mean_broadening_params, wn_bin_centers, wn_bin_widths, sw_sum,
                     lsw_mean_e_lower, store, store_x)
        rc = eng._lib.ansfm_lbl_accum_add_pseudo_continuum(
            eng._ctx, int(lineshape_id), float(t_ref), float(p_ref), _ptr(a.q), float(isotopic_abundance), float(isotopic_mass),
            a.M, _ptr(a.mmf), a.N, _ptr(a.bp), _ptr(a.c), _ptr(a.w), _ptr(a.sw), _ptr(a.el), _ptr(store), _ptr(store_x),
            int(n_neighbour_bins))
        eng._check(rc, "lbl_accum_add_pseudo_continuum")
        return self

    def numpy(self):
        """the sum as a new (L, nw) host array"""
        self._live()
        out = np.empty((self.L, self.nw))
        self._eng._check(self._eng._lib.ansfm_lbl_accum_read(self._eng._ctx, _ptr(out)), "lbl_accum_read")
        return out

    def device_ptr(self):
        """address of the (L, nw) float64 buffer in HBM, after the adds queued so far have finished"""
        self._live()
        ptr = C.c_void_p(); L = C.c_int(); nw = C.c_int()
        self._eng._check(self._eng._lib.ansfm_lbl_accum_device_ptr(self._eng._ctx, C.byref(ptr), C.byref(L), C.byref(nw)),
                         "lbl_accum_device_ptr")
        return int(ptr.value)

    def torch(self):
        """the buffer itself as a torch tensor (L, nw) on the engine's device: no copy, so a later add shows in it (once the
        engine's stream has finished it: `eng.synchronize()`), and it is valid only until the engine's next accumulator"""
        import torch
        return torch.as_tensor(_DeviceArray(self.device_ptr(), (self.L, self.nw), self), device="cuda:%d" % self._eng.device)
