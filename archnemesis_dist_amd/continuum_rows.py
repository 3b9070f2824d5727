"""The continuum of the forward models of a numerical Jacobian, once per distinct layer.

A state vector element touches a few layers; everywhere else TAUCIA, TAUDUST, TAURAY, TAUSCAT and the aerosol fractions of a
perturbed state are the first state's, bit for bit.  `ContinuumRows` keeps the first state's L layers as rows 0 .. L-1 and, of
every later state, only the layers whose column differs from the first state's in any bit of any of the five arrays, with the
map `cont_row[state, layer] -> row`.  That is the form `AnsfmEngine.cirsrad_ck_scatter_batch_rows` takes: rows are stored
wavenumber fastest, (R, NWAVE) and (R, NDUST, NWAVE).  States are added one at a time, so a caller can drop each state's dense
arrays as soon as they are packed.
"""
import numpy as np

NAMES = ("TAUCIA", "TAUDUST", "TAURAY", "TAUSCAT", "FRAC")


def _bits(a):
    return a.view(np.uint64)


class ContinuumRows:
    def __init__(self, L, ncont):
        self.L = int(L)
        self.ncont = int(ncont)
        self.W = None
        self._first = None            # the first state's arrays, (W, L) / (W, ncont, L), or None where the caller gave None
        self._blocks = None           # per array: list of row blocks (k, W) / (k, ncont, W)
        self._cont_row = []
        self._R = 0
        self._packed = None

    # ---- packing --------------------------------------------------------------------------------------------------
    def _checked(self, arrays):
        if len(arrays) != 5:
            raise ValueError("add_state takes TAUCIA, TAUDUST, TAURAY, TAUSCAT, FRAC")
        out = []
        for name, a in zip(NAMES, arrays):
            if a is not None and name == "FRAC" and self.ncont == 0:
                a = None
            if a is None:
                out.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=np.float64)
            want = (self.ncont, self.L) if name == "FRAC" else (self.L,)
            if a.ndim != len(want) + 1 or a.shape[1:] != want:
                raise ValueError(f"{name} must be (NWAVE, {', '.join(str(v) for v in want)}), got {a.shape}")
            if self.W is None:
                self.W = a.shape[0]
            if a.shape[0] != self.W:
                raise ValueError(f"{name} has {a.shape[0]} wavenumbers, the first state's arrays have {self.W}")
            out.append(a)
        return out

    @staticmethod
    def _rows_of(a, layers):
        """(W, L) -> (k, W); (W, ncont, L) -> (k, ncont, W): the columns of `layers`, wavenumber fastest"""
        return np.ascontiguousarray(np.moveaxis(a[..., layers], -1, 0).swapaxes(-1, 1) if a.ndim == 3
                                    else a[:, layers].T)

    def add_state(self, TAUCIA, TAUDUST, TAURAY, TAUSCAT, FRAC):
        """One state's arrays in the reference's layouts: (NWAVE, NLAY) each, FRAC (NWAVE, NDUST, NLAY); None = zeros (the
        same arrays must be None in every state).  Returns the state's row of `cont_row`."""
        arrays = self._checked((TAUCIA, TAUDUST, TAURAY, TAUSCAT, FRAC))
        self._packed = None
        if self._first is None:
            self._first = [None if a is None else a.copy() for a in arrays]
            self._blocks = [None if a is None else [self._rows_of(a, np.arange(self.L))] for a in arrays]
            row = np.arange(self.L, dtype=np.int32)
            self._R = self.L
            self._cont_row.append(row)
            return row
        changed = np.zeros(self.L, dtype=bool)
        for name, a, a0 in zip(NAMES, arrays, self._first):
            if (a is None) != (a0 is None):
                raise ValueError(f"{name} is None in one state and an array in another")
            if a is not None:
                d = _bits(a) != _bits(a0)                       # -0.0 vs 0.0 and NaN payloads count
                changed |= d.any(axis=tuple(range(d.ndim - 1)))
        layers = np.flatnonzero(changed)
        row = np.arange(self.L, dtype=np.int32)
        row[layers] = self._R + np.arange(layers.size, dtype=np.int32)
        if layers.size:
            for a, blocks in zip(arrays, self._blocks):
                if a is not None:
                    blocks.append(self._rows_of(a, layers))
        self._R += int(layers.size)
        self._cont_row.append(row)
        return row

    # ---- the packed form ------------------------------------------------------------------------------------------
    def _pack(self):
        if self._packed is None:
            if self._first is None:
                raise ValueError("no state added")
            self._packed = [None if b is None else (b[0] if len(b) == 1 else np.concatenate(b, axis=0)) for b in self._blocks]
            for i, b in enumerate(self._blocks):                # keep one copy
                if b is not None:
                    self._blocks[i] = [self._packed[i]]
        return self._packed

    @property
    def n_states(self):
        return len(self._cont_row)

    @property
    def R(self):
        return self._R

    @property
    def cont_row(self):
        return np.stack(self._cont_row).astype(np.int32, copy=False)

    TAUCIA_rows = property(lambda self: self._pack()[0])
    TAUDUST_rows = property(lambda self: self._pack()[1])
    TAURAY_rows = property(lambda self: self._pack()[2])
    TAUSCAT_rows = property(lambda self: self._pack()[3])
    lfrac_rows = property(lambda self: self._pack()[4])

    def rows(self):
        """(cont_row, TAUCIA_rows, TAUDUST_rows, TAURAY_rows, TAUSCAT_rows, lfrac_rows)"""
        return (self.cont_row,) + tuple(self._pack())

    @property
    def nbytes(self):
        return self.cont_row.nbytes + sum(a.nbytes for a in self._pack() if a is not None)

    def slice_waves(self, lo, hi):
        """The five row arrays cut to the wavenumbers [lo, hi) (one rank's slice of a sharded axis); cont_row is unchanged."""
        return tuple(None if a is None else np.ascontiguousarray(a[..., lo:hi]) for a in self._pack())

    def expand(self):
        """The dense arrays: TAUCIA, TAUDUST, TAURAY, TAUSCAT (n, NWAVE, NLAY), FRAC (n, NWAVE, NDUST, NLAY) (None stays None)"""
        return expand_rows(*self.rows())


def expand_rows(cont_row, *rows):
    """dense[m, w, l] = rows[cont_row[m, l], w] for (R, NWAVE) arrays, dense[m, w, c, l] = rows[cont_row[m, l], c, w] for
    (R, NDUST, NWAVE) ones; None stays None"""
    cr = np.asarray(cont_row)
    out = []
    for a in rows:
        if a is None:
            out.append(None)
        elif a.ndim == 2:
            out.append(np.ascontiguousarray(a[cr].transpose(0, 2, 1)))          # (n, L, W) -> (n, W, L)
        else:
            out.append(np.ascontiguousarray(a[cr].transpose(0, 3, 2, 1)))       # (n, L, C, W) -> (n, W, C, L)
    return tuple(out)


def pack_batch(TAUCIA, TAUDUST, TAURAY, TAUSCAT, lfrac, L=None, ncont=None):
    """The dense arrays of a batch -- (n, NWAVE, NLAY) or None, lfrac (n, NWAVE, NDUST, NLAY) or None -- packed state by state"""
    arrays = [None if a is None else np.asarray(a) for a in (TAUCIA, TAUDUST, TAURAY, TAUSCAT, lfrac)]
    given = [a for a in arrays if a is not None]
    if not given:
        raise ValueError("pack_batch: every array is None")
    n = given[0].shape[0]
    L = given[0].shape[-1] if L is None else L
    ncont = (arrays[4].shape[2] if arrays[4] is not None else 0) if ncont is None else ncont
    pk = ContinuumRows(L, ncont)
    for m in range(n):
        pk.add_state(*(None if a is None else a[m] for a in arrays))
    return pk


def rows_kwargs(inputs):
    """The keyword arguments of `cirsrad_ck_scatter_batch` -> those of `cirsrad_ck_scatter_batch_rows` (the continuum packed)"""
    out = dict(inputs)
    dense = [out.pop(k) for k in ("TAUCIA", "TAUDUST", "TAURAY", "TAUSCAT", "lfrac")]
    pk = pack_batch(*dense, L=np.asarray(inputs["lay_press_pa"]).shape[1])
    out.update(zip(("cont_row", "TAUCIA_rows", "TAUDUST_rows", "TAURAY_rows", "TAUSCAT_rows", "lfrac_rows"), pk.rows()))
    return out
