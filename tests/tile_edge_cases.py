"""Seeded cases at the tile, chunk and clamp edges of k_ils_conv, k_kdist_gather / k_kdist_quantiles and k_gemm_f64
(NumPy only; tests/test_tile_edges_host.py measures their bounds, tests/test_tile_edges_gpu.py runs them on the kernels,
oracle/gen_golden_tile_edges.py records the reference's ILS results in tests/golden/tile_edges.npz).

k_ils_conv stages its window in chunks of 128 points and takes 128 columns per block; k_kdist_quantiles scans a bin in 256
chunks of ceil(n / 256) points; k_gemm_f64 works on 64 x 64 tiles of C with K in chunks of 16.  The cases are the smallest
shapes that sit on, one below and one above each of these numbers.

Every adapter below returns the same thing for the same case, whoever computes it: run_ils(api, case) -> (yout, gradout or
None) with api the oracle module, the engine, or LD (this module's np.longdouble restatement of the same formulas)."""
import numpy as np

LD = "longdouble"
ld = np.longdouble

# ---- ILS convolution ---------------------------------------------------------------------------------------------------
NWAVE = 700
FIL_CENTRES = (2000.02, 2001.3, 2003.5, 2004.9, 2006.965)     # all strictly inside the grid, as conv / convg need
FIL_HALVES = (0.015, 0.635, 1.285, 2.0, 0.02)
FIL_NFIL = (2, 3, 7, 5, 2)
FIL_COUNTS = (3, 127, 257, 400, 4)            # points of the grid inside each filter (asserted on the host)
NFILMAX = 7
# FWHM per ISHAPE: square FWHM wide (128 points), triangle and gradient-Hamming 2 FWHM (129), gaussian +-1.8 FWHM, Hanning +-3 FWHM
SHAPE_FWHM = {0: 1.28, 1: 0.645, 2: 0.5, 3: 0.645, 4: 0.3}
SHAPE_VCONV = (2003.5, 2001.117, 2005.731)
SHAPE_COUNTS = {0: 128, 1: 129}               # at SHAPE_VCONV[0]


def ils_grid(repeat=False):
    rng = np.random.default_rng(20240)
    vwave = np.sort(2000.0 + 0.01 * np.arange(NWAVE) + rng.uniform(-3e-3, 3e-3, NWAVE))
    if repeat:
        vwave[350:353] = vwave[350]           # three equal wavenumbers inside the windows around 2003.5 (the grid stays ascending)
    return vwave


def _ils_columns(ny, nx, seed):
    rng = np.random.default_rng(seed)
    y = 1e-7 * rng.uniform(1.0, 2.0, (NWAVE, ny))
    dydx = rng.normal(size=(NWAVE, ny, nx)) * 10.0 ** rng.uniform(-10, -7, (1, 1, nx)) if nx else None
    if ny == 1:
        return y[:, 0], (None if dydx is None else dydx[:, 0, :])
    return y, dydx


def ils_filters():
    """five tabulated filters, nfil = (2, 3, 7, 5, 2) under nfilmax = 7; the 257-point one is 0 at two interior nodes"""
    rng = np.random.default_rng(20241)
    nc = len(FIL_CENTRES)
    nfil = np.array(FIL_NFIL, dtype=np.int32)
    vfil = np.zeros((NFILMAX, nc)); afil = np.zeros((NFILMAX, nc))
    for j in range(nc):
        vfil[:nfil[j], j] = np.linspace(FIL_CENTRES[j] - FIL_HALVES[j], FIL_CENTRES[j] + FIL_HALVES[j], nfil[j])
        afil[:nfil[j], j] = rng.uniform(0.1, 1.0, nfil[j])
    afil[2, 2] = 0.0; afil[4, 2] = 0.0
    return dict(vconv=np.array(FIL_CENTRES), nfil=nfil, vfil=vfil, afil=afil)


def placement_filters(vwave):
    """two-node filters whose windows begin at index 0, end at nwave - 1, hold one point, hold none (between two grid
    points) and lie outside the grid; nfilmax = 4 with the unused rows left at 0"""
    mid = 0.5 * (vwave[399] + vwave[400])
    edges = [(vwave[0] - 0.5, vwave[5] + 1e-4), (vwave[-6] - 1e-4, vwave[-1] + 0.5), (vwave[200] - 1e-4, vwave[200] + 1e-4),
             (mid - 1e-5, mid + 1e-5), (vwave[-1] + 1.0, vwave[-1] + 2.0), (vwave[0], vwave[2])]
    nc = len(edges)
    vfil = np.zeros((4, nc)); afil = np.zeros((4, nc))
    for j, (a, b) in enumerate(edges):
        vfil[:2, j] = (a, b); afil[:2, j] = (0.25 + 0.1 * j, 1.0)
    return dict(vconv=np.array([0.5 * (a + b) for a, b in edges]), nfil=np.full(nc, 2, dtype=np.int32), vfil=vfil, afil=afil)


PLACEMENT_COUNTS = (6, 6, 1, 0, 0, 3)


def window_counts(vwave, f):
    return tuple(int(((vwave >= f["vfil"][0, j]) & (vwave <= f["vfil"][f["nfil"][j] - 1, j])).sum()) for j in range(f["nfil"].size))


def shape_window_count(vwave, ishape, vcen, fwhm):
    v1, v2 = (vcen - 0.5 * fwhm, vcen - 0.5 * fwhm + fwhm) if ishape == 0 else (vcen - fwhm, vcen + fwhm)
    return int(((vwave >= v1) & (vwave <= v2)).sum())


def ils_cases():
    """name -> dict(kind = 'shape' | 'fil' | 'bracket' | 'integrate', vwave, y, dydx, vconv, [ishape, fwhm | nfil, vfil, afil])"""
    vw = ils_grid()
    F = ils_filters()
    out = {}
    for nx in (127, 128, 129):                                         # nx + ny = 128, 129, 130 columns
        y, d = _ils_columns(1, nx, 100 + nx)
        out["fil-%d" % (nx + 1)] = dict(kind="fil", vwave=vw, y=y, dydx=d, **F)
    y1, d1 = _ils_columns(1, 129, 7)
    y3, d3 = _ils_columns(3, 42, 8)                                    # ngeom: 42 * 3 + 3 = 129 columns
    out["fil-y"] = dict(kind="fil", vwave=vw, y=y1, dydx=None, **F)
    out["fil-ngeom"] = dict(kind="fil", vwave=vw, y=y3, dydx=None, **F)
    out["filg-ngeom"] = dict(kind="fil", vwave=vw, y=y3, dydx=d3, **F)
    out["bracket-y"] = dict(kind="bracket", vwave=vw, y=y1, dydx=None, **F)
    out["bracket-g"] = dict(kind="bracket", vwave=vw, y=y1, dydx=d1, **F)
    out["intf-1"] = dict(kind="integrate", vwave=vw, y=y1, dydx=None, **F)
    out["intfg-1"] = dict(kind="integrate", vwave=vw, y=y1, dydx=d1, **F)
    out["intf-3"] = dict(kind="integrate", vwave=vw, y=y3, dydx=None, **F)
    out["intfg-3"] = dict(kind="integrate", vwave=vw, y=y3, dydx=d3, **F)
    vc = np.array(SHAPE_VCONV)
    for ishape in range(5):
        sh = dict(vwave=vw, vconv=vc, ishape=ishape, fwhm=SHAPE_FWHM[ishape])
        out["shape%d-g" % ishape] = dict(kind="shape", y=y1, dydx=d1, **sh)
        out["shape%d-y" % ishape] = dict(kind="shape", y=y1, dydx=None, **sh)
        out["shape%d-ngeom" % ishape] = dict(kind="shape", y=y3, dydx=d3, **sh)
    P = placement_filters(vw)
    out["place-fil"] = dict(kind="fil", vwave=vw, y=y1, dydx=d1, **P)
    out["place-intf"] = dict(kind="integrate", vwave=vw, y=y3, dydx=d3, **P)
    # square and triangle windows over the first and the last points of the grid, around one point, and outside the grid
    pv = np.array([vw[0], vw[-1], vw[200], vw[-1] + 5.0])
    out["place-shape0"] = dict(kind="shape", vwave=vw, y=y1, dydx=d1, vconv=pv, ishape=0, fwhm=0.05)
    out["place-shape1"] = dict(kind="shape", vwave=vw, y=y1, dydx=d1, vconv=pv, ishape=1, fwhm=0.05)
    out["place-point"] = dict(kind="shape", vwave=vw, y=y1, dydx=d1, vconv=pv[2:3], ishape=0, fwhm=2e-4)
    vr = ils_grid(repeat=True)
    out["repeat-fil"] = dict(kind="fil", vwave=vr, y=y1, dydx=d1, **F)
    out["repeat-intf"] = dict(kind="integrate", vwave=vr, y=y1, dydx=d1, **F)
    out["repeat-shape1"] = dict(kind="shape", vwave=vr, y=y1, dydx=d1, vconv=vc, ishape=1, fwhm=SHAPE_FWHM[1])
    return out


def ils_exact_case():
    """ISHAPE 0 with integer-valued y and dydx in [-8, 8]: sums and counts are exact, the quotient is correctly rounded"""
    rng = np.random.default_rng(20242)
    y = rng.integers(-8, 9, NWAVE).astype(float)
    d = rng.integers(-8, 9, (NWAVE, 129)).astype(float)
    return dict(kind="shape", vwave=ils_grid(), y=y, dydx=d, vconv=np.array(SHAPE_VCONV + (2000.0, 2006.99)), ishape=0,
                fwhm=SHAPE_FWHM[0])


def is_mean(case):
    return case["kind"] != "integrate"


def _ld_interp(x, xp, fp):
    """np.interp in np.longdouble: fp[j] + slope (x - xp[j]) with j the last xp[j] <= x, the ends clamped"""
    x = np.asarray(x, ld); xp = np.asarray(xp, ld); fp = np.asarray(fp, ld)
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, xp.size - 2)
    with np.errstate(all="ignore"):
        r = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (x - xp[j]) + fp[j]
    r = np.where(x == xp[j], fp[j], r)
    r = np.where(x >= xp[-1], fp[-1], r)
    return np.where(x <= xp[0], fp[0], r)


def _ld_shape_weight(ishape, v, vcen, fwhm, sig):
    v = v.astype(ld); vcen = ld(vcen); fwhm = ld(fwhm)
    if ishape == 0:
        return np.ones_like(v)
    if ishape == 1:
        return 1 - np.abs(v - vcen) / fwhm
    if ishape == 2:
        return np.exp(-((v - vcen) / sig) ** 2)
    if ishape == 3:
        a = ld(0.907) / fwhm; k = v - vcen; pi = ld(np.pi)
        with np.errstate(all="ignore"):
            f = a * (ld(1.08) - ld(0.64) * a ** 2 * k ** 2) * np.sin(2 * pi * a * k) / ((1 - 4 * a ** 2 * k ** 2) * (2 * pi * a * k))
        return np.where(k != 0, f, a * ld(1.08))
    return np.zeros_like(v)


def _ils_longdouble(case):
    from oracle import oracle as orc
    vw = case["vwave"]
    grad = case["dydx"] is not None
    ngeom = case["y"].ndim == 2
    cols, ng, nx = orc._ils_cols(case["y"], case["dydx"], ngeom)
    cols = cols.astype(ld)
    nconv = case["vconv"].size
    out = np.zeros((nconv, cols.shape[1]), ld)
    for j in range(nconv):
        if case["kind"] == "shape":
            # the window is decided in float64, as everywhere: it is a selection of points, not arithmetic
            v1, v2, sig = orc._ils_window(case["ishape"], case["vconv"][j], case["fwhm"], grad, ngeom)
            idx = np.where((vw >= v1) & (vw <= v2))[0]
            sig = ld(0.5) * ld(case["fwhm"]) / np.sqrt(np.log(ld(2)))
            f = _ld_shape_weight(case["ishape"], vw[idx], case["vconv"][j], case["fwhm"], sig)
        else:
            n = int(case["nfil"][j]); xp = case["vfil"][:n, j]; fp = case["afil"][:n, j]
            idx = np.where((vw >= xp[0]) & (vw <= xp[-1]))[0]
            if case["kind"] == "bracket":
                idx = np.arange(np.where(vw < xp[0])[0][-1], np.where(vw > xp[-1])[0][0] + 1)
            f = _ld_interp(vw[idx], xp, fp)
        if case["kind"] == "integrate":
            v = vw[idx].astype(ld); fy = cols[idx] * f[:, None]
            out[j] = ((v[1:] - v[:-1])[:, None] * (fy[1:] + fy[:-1]) / 2).sum(axis=0) if idx.size > 1 else 0
        else:
            keep = f > 0
            with np.errstate(all="ignore"):
                out[j] = (f[keep, None] * cols[idx][keep]).sum(axis=0) / f[keep].sum()
    return orc._ils_split(out, ng, nx, grad, ngeom) if grad else (orc._ils_split(out, ng, nx, grad, ngeom), None)


def run_ils(api, c):
    """(yout, gradout or None) of one case from the oracle module, the engine, or the longdouble restatement (api = LD)"""
    if api == LD:
        return _ils_longdouble(c)
    vw, y, d, vc = c["vwave"], c["y"], c["dydx"], c["vconv"]
    nw, nc = vw.size, vc.size
    ngeom = y.ndim == 2
    is_oracle = not hasattr(api, "lblconvg_fil")
    f = (c["nfil"], c["vfil"], c["afil"]) if c["kind"] != "shape" else None
    with np.errstate(all="ignore"):
        if c["kind"] == "integrate":
            r = api.integrate_filter(nw, vw, y, nc, vc, *f, dydx=d)
        elif is_oracle:
            r = (api.lblconv(nw, vw, y, nc, vc, c["ishape"], c["fwhm"], dydx=d, ngeom=ngeom) if f is None else
                 api.lblconv_fil(nw, vw, y, nc, vc, *f, dydx=d, ngeom=ngeom, bracket=c["kind"] == "bracket"))
        elif c["kind"] == "bracket":
            r = api.conv_fil(vw, y, d, nc, vc, *f)
        else:
            name = "lblconv" + ("g" if d is not None else "") + ("_fil" if f else "") + ("_ngeom" if ngeom else "")
            a = (nw, vw, y) + (() if d is None else (d,)) + (nc, vc) + (f if f else (c["ishape"], c["fwhm"]))
            r = getattr(api, name)(*a)
    return r if d is not None else (r, None)


def ils_deviation(got, want, mean):
    """(spectra, gradients): largest relative deviation point by point; the gradients of the integrals, which cancel, relative
    to the largest gradient.  NaN where both are NaN counts as equal, anywhere else as infinite."""
    out = []
    for k, (a, b) in enumerate(zip(got, want)):
        if b is None:
            out.append(0.0)
            continue
        a = np.asarray(a, ld); b = np.asarray(b, ld)
        if not np.array_equal(np.isnan(a), np.isnan(b)):
            out.append(np.inf)
            continue
        m = ~np.isnan(b)
        if not m.any() or not np.any(b[m]):
            out.append(0.0 if np.array_equal(a[m], b[m]) else np.inf)
            continue
        scale = np.abs(b[m]) if (mean or k == 0) else np.abs(b[m]).max()
        with np.errstate(all="ignore"):
            r = np.abs(a[m] - b[m]) / scale
        r = np.where(a[m] == b[m], 0, r)
        out.append(float(r.max()))
    return tuple(out)


ILS_CAPS = {True: (1e-12, 1e-11), False: (1e-12, 1e-12)}      # is_mean -> (spectra, gradients): the existing tests' tolerances


# ---- k-distribution ----------------------------------------------------------------------------------------------------
NCALC = 1100
BIN_SIZES = (1, 2, 3, 255, 256, 257, 511, 512, 513, 1000)
BIN_STARTS = (40, 41, 300, 120, 250, 333, 400, 90, NCALC - 513, 0)      # overlapping; one from index 0, one to ncalc - 1
G9 = np.array([0.0, 1e-9, 0.013, 0.25, 0.5, 0.75, 0.987, 1.0 - 1e-9, 1.0])
KDIST_CAP = 1e-10


def g300():
    g = np.sort(np.random.default_rng(20250).uniform(0.0, 1.0, 300))
    g[0], g[-1] = 0.0, 1.0
    return g


def kdist_grid():
    rng = np.random.default_rng(20251)
    wave = 1000.0 + 0.01 * np.arange(NCALC)
    return wave, 10.0 ** rng.uniform(-26, -20, NCALC)


def _bins(wave, starts, sizes):
    lo = np.array([wave[a] - 1e-4 for a in starts]); hi = np.array([wave[a + n - 1] + 1e-4 for a, n in zip(starts, sizes)])
    return lo, hi


def bin_counts(wave, lo, hi):
    return tuple(int(((wave >= a) & (wave <= b)).sum()) for a, b in zip(lo, hi))


def _narrow_filter(lo, hi, afil=(0.0, 1.0, 0.5, 0.0)):
    """four nodes per bin, narrower than the bin: the points beyond it on either side get afil[0] = afil[3] = 0 through the
    clamps.  The two points of the n = 2 bin would both lie outside; that bin gets a filter wider than itself."""
    nbin = lo.size
    cen = 0.5 * (lo + hi)
    h = 0.3 * (hi - lo) + 1e-3
    two_points = (hi - lo > 0.005) & (hi - lo < 0.015)
    h = np.where(two_points, 0.02, h)
    dfil = np.array([-h, -0.2 * h, 0.4 * h, h])
    return cen, np.full(nbin, 4, dtype=np.int32), dfil, np.tile(np.array(afil)[:, None], (1, nbin))


def kdist_cases():
    """name -> dict(wave, kabs, lo, hi, fil): every bin is run alone and all of them in one call, the 257-point bin twice"""
    wave, k = kdist_grid()
    starts = BIN_STARTS + (BIN_STARTS[5],); sizes = BIN_SIZES + (BIN_SIZES[5],)
    lo, hi = _bins(wave, starts, sizes)
    out = {"plain": dict(wave=wave, kabs=k, lo=lo, hi=hi, fil=None),
           "filter": dict(wave=wave, kabs=k, lo=lo, hi=hi, fil=_narrow_filter(lo, hi))}
    # all weights 0: 0/0 at every ordinate for 50 points; np.interp on a single point returns it whatever its abscissa is
    zlo, zhi = _bins(wave, (500, 700), (50, 1))
    out["zero-weight"] = dict(wave=wave, kabs=k, lo=zlo, hi=zhi, fil=_narrow_filter(zlo, zhi, (0.0, 0.0, 0.0, 0.0)))
    # tied k with EQUAL weights: the cumulative weights do not depend on the order inside a run of equal k.  With unequal
    # weights inside a run the reference's np.argsort (quicksort, not stable) leaves the order, and so the result, undefined;
    # the oracle and the radix sort are both stable.
    tied = np.round(np.random.default_rng(20252).uniform(0, 5, NCALC)) * 1e-22
    tlo, thi = _bins(wave, (100, 300), (257, 600))
    out["ties"] = dict(wave=wave, kabs=tied, lo=tlo, hi=thi, fil=None)
    slo, shi = _bins(wave, (BIN_STARTS[8], 10), (513, 300))
    for name, pos, val in (("inf", 700, np.inf), ("nan-pos", 800, np.copysign(np.nan, 1.0)), ("nan-neg", 800, np.copysign(np.nan, -1.0))):
        kk = k.copy(); kk[pos] = val
        out[name] = dict(wave=wave, kabs=kk, lo=slo, hi=shi, fil=None)
    return out


def one_bin(c, b):
    f = c["fil"]
    s = slice(b, b + 1)
    return dict(c, lo=c["lo"][s], hi=c["hi"][s], fil=None if f is None else (f[0][s], f[1][s], f[2][:, s], f[3][:, s]))


def run_kdist(api, c, g):
    if api == LD:
        return _kdist_longdouble(c, g)
    with np.errstate(all="ignore"):
        return api.kdist_bins(c["wave"], c["kabs"], c["lo"], c["hi"], g, c["fil"])


def bin_weights(c, b):
    """weights of the points of bin b in grid order (float64, as the oracle forms them)"""
    wave = c["wave"]
    m = (wave >= c["lo"][b]) & (wave <= c["hi"][b])
    if c["fil"] is None:
        return np.ones(int(m.sum()))
    cen, nfil, dfil, afil = c["fil"]
    return np.interp(wave[m] - cen[b], dfil[:nfil[b], b], afil[:nfil[b], b])


def _kdist_longdouble(c, g):
    wave, kabs = c["wave"], c["kabs"]
    out = np.zeros((c["lo"].size, g.size), ld)
    for b in range(c["lo"].size):
        m = (wave >= c["lo"][b]) & (wave <= c["hi"][b])
        idx = np.argsort(kabs[m], kind="stable")
        ks = kabs[m][idx].astype(ld)
        if c["fil"] is None:
            w = np.ones(ks.size, ld)
        else:
            cen, nfil, dfil, afil = c["fil"]
            w = _ld_interp(wave[m][idx].astype(ld) - ld(cen[b]), dfil[:nfil[b], b], afil[:nfil[b], b])
        wdv = w * (ld(wave[1]) - ld(wave[0]))
        with np.errstate(all="ignore"):
            gs = np.cumsum(wdv) / wdv.sum()
            if ks.size == 1 or np.isnan(gs).all():
                out[b] = ks[0] if ks.size == 1 else np.nan
                continue
            j = np.clip(np.searchsorted(gs, g.astype(ld), side="right") - 1, 0, ks.size - 2)
            r = (ks[j + 1] - ks[j]) / (gs[j + 1] - gs[j]) * (g - gs[j]) + ks[j]
        r = np.where(g == gs[j], ks[j], r)
        r = np.where(g >= gs[-1], ks[-1], r)
        out[b] = np.where(g < gs[0], ks[0], r)
    return out


def kdist_deviation(got, want):
    a = np.asarray(got, ld); b = np.asarray(want, ld)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return np.inf
    m = ~np.isnan(b) & (a != b)
    if not m.any():
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m])))


# ---- gradient maps (k_gemm_f64 behind map2pro / map2xvec) ---------------------------------------------------------------
#             W  NPRO LIMAX NPATH NX NVMR NDUST
MAP_SHAPES = ((1, 1, 1, 1, 1, 1, 0),
              (63, 15, 3, 1, 64, 2, 1),
              (64, 16, 15, 3, 65, 1, 1),
              (65, 17, 16, 1, 70, 2, 0),
              (129, 64, 17, 1, 1, 1, 2),
              (65, 65, 16, 3, 64, 1, 1),
              (64, 130, 1, 1, 65, 1, 0),
              (1, 64, 33, 3, 1, 3, 2),
              (63, 65, 17, 3, 70, 2, 2),
              (129, 130, 33, 3, 70, 2, 1))        # W > 64, NPRO > 64 and NPATH = 3 together: the largest
MAP_VALUES = dict(W=(1, 63, 64, 65, 129), NPRO=(1, 15, 16, 17, 64, 65, 130), LIMAX=(1, 3, 15, 16, 17, 33), NPATH=(1, 3),
                  NX=(1, 64, 65, 70))
MAP_NEGATIVE_LAYINC = (2, 5, 9)                   # cases whose LAYINC holds Python-style negative indices
MAP_INCPAR_SUBSET = (8, 9)                        # cases that list the para-H2 slot after another parameter


def map_case(i, real=False):
    W, NPRO, LIMAX, NPATH, NX, NVMR, NDUST = MAP_SHAPES[i]
    rng = np.random.default_rng(20260 + i + (100 if real else 0))
    NPAR = NVMR + 2 + NDUST
    NLAY = LIMAX + 4
    draw = (lambda *s: rng.normal(size=s)) if real else (lambda *s: rng.integers(-8, 9, s).astype(float))
    LAYINC = rng.integers(0, NLAY, (LIMAX, NPATH)).astype(np.int32)
    if i in MAP_NEGATIVE_LAYINC:
        LAYINC[::2] -= NLAY
        assert (LAYINC < 0).any() and (LAYINC >= -NLAY).all()
    INCPAR = (1, NPAR - 1, 0) if i in MAP_INCPAR_SUBSET else (-1,)
    return dict(W=W, NPRO=NPRO, LIMAX=LIMAX, NPATH=NPATH, NX=NX, NVMR=NVMR, NDUST=NDUST, NPAR=NPAR, NLAY=NLAY, LAYINC=LAYINC,
                INCPAR=INCPAR, dSPECIN=draw(W, NPAR, LIMAX, NPATH), DTE=draw(NLAY, NPRO), DAM=draw(NLAY, NPRO),
                DCO=draw(NLAY, NPRO), xmap=draw(NX, NPAR, NPRO))


def map2pro_args(c):
    return (c["W"], c["NVMR"], c["NDUST"], c["NPRO"], c["NPATH"], c["LIMAX"], c["LAYINC"], c["DTE"], c["DAM"], c["DCO"])


def map2xvec_args(c):
    return (c["W"], c["NVMR"], c["NDUST"], c["NPRO"], c["NPATH"], c["NX"], c["xmap"])


def map_longdouble(c, pro=None):
    """(map2pro, |A|.|B| of it, map2xvec of `pro` (default: the float64 rounding of the longdouble map2pro), |A|.|B| of that)
    in np.longdouble, for the bound 2 K 2^-53 (|A|.|B|) of a float64 product of depth K"""
    A = c["dSPECIN"].astype(ld)
    P = np.zeros((c["W"], c["NPAR"], c["NPRO"], c["NPATH"]), ld); Pabs = P.copy()
    inc = range(c["NPAR"]) if c["INCPAR"][0] == -1 else c["INCPAR"]
    for p in range(c["NPATH"]):
        last = None
        for par in inc:
            M = c["DAM"] if par <= c["NVMR"] - 1 else c["DTE"] if par <= c["NVMR"] else c["DCO"] if par <= c["NVMR"] + c["NDUST"] else None
            if M is not None:
                B = M[c["LAYINC"][:, p], :].astype(ld)
                last = (A[:, par, :, p] @ B, np.abs(A[:, par, :, p]) @ np.abs(B))
            P[:, par, :, p], Pabs[:, par, :, p] = last
    pro = P.astype(float) if pro is None else pro
    a = np.moveaxis(pro.astype(ld), 3, 1).reshape(c["W"], c["NPATH"], -1)
    x = c["xmap"].astype(ld).reshape(c["NX"], -1).T
    return P, Pabs, a @ x, np.abs(a) @ np.abs(x)
