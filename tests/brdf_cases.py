"""Surface reflection (Surface_0.calc_Hapke_BRDF :1292, calc_OrenNayar_BRDF :1743, Surface_0.calc_BRDF :916 and
ForwardModel_0.calc_brdf_matrix :5168): the cases of tests/golden/brdf.npz (tools/golden/gen_golden_brdf.py runs the
reference on them) and the project's own NumPy restatement -- the written-down contract of the kernels in
csrc/ansfm_surface_kernels.hip.h.

`params` holds one row per parameter, (npar, nwave): LOWBC 1 the albedo; LOWBC 2 the ten arguments of calc_Hapke_BRDF in
its order (w, K, BS0, hs, BC0, hc, ROUGHNESS, G1, G2, F); LOWBC 3 (A, ROUGHNESS).

Hapke, per point (i, e, phi_nemesis) in degrees, every operation in the reference's order:
  * phi = 180 - phi_nemesis folded into [0, 180] (phix); e >= 90 or i >= 90 gives 0
  * cg = mu mu0 + sqrt(1 - mu^2) sqrt(1 - mu0^2) cos(phix) clamped to [0, 1]; g = arccos(cg) in degrees
  * gamma = sqrt(1 - w), r0 = (1 - gamma)/(1 + gamma), theta_bar = ROUGHNESS (1 - r0), chi = 1/sqrt(1 + pi tan^2 theta_bar)
  * fphi = exp(-2 |tan(phix / 2)|), 0 iff |phix| == 180
  * E1(x) = exp(-2/pi / tan theta_bar / tan x), E2(x) = exp(-1/pi / tan^2 theta_bar / tan^2 x), both 0 iff theta_bar == 0 or
    x == 0; nu(x) = chi (cos x + sin x tan theta_bar E2(x) / (2 - E1(x)))
  * with s the smaller of (i, e) -- i when they are equal -- and l the other (the reference's two branches are one formula
    with the roles exchanged):  eff_s = chi (cos s + sin s tan theta_bar (cos phix E2(l) + sin^2(phix/2) E2(s)) / den),
    eff_l = chi (cos l + sin l tan theta_bar (E2(l) - sin^2(phix/2) E2(s)) / den), den = 2 - E1(l) - phix/pi E1(s)
  * S = mueff/nu(e) mu0/nu(i) chi / (1 - fphi + fphi chi cos s / nu(s))
  * Bs, Bc from tan(g/2); H(x) the Ambartsumian-Chandrasekhar function; the double Henyey-Greenstein phase
  * BRDF = K w/(4 pi) mu0eff/(mu0eff + mueff) (phase (1 + Bs) + H0e He - 1) (1 + Bc) S / mu0
Each transcendental is evaluated once per distinct argument (cos i, sin i, tan i, tan theta_bar, cos phix, tan(g/2), ...),
which gives the bits of the reference's repeated evaluations.  The squares are products.

The matrix: for every (wavenumber, j, i), the sum over k = 0 .. NPHI in order of wphi[k] BRDF cos(ic k dphi), wphi =
dphi / 2 pi halved at both ends, at the angles arccos(MU[::-1]) -- into BRDF_mat[w][i][j][ic].  LAMBERTIAN: plane 0 is
albedo / pi, set, not integrated.  Every other LOWBC: zeros.

`ulp`: an object called on the result of every cos / sin / tan / exp / log / arccos / sqrt / pow and on cg -- the identity
for the restatement itself; `Nudge` moves each result by one np.nextafter to measure what one ulp in those is worth."""
import numpy as np

HAPKE_NAMES = ("w", "K", "BS0", "hs", "BC0", "hc", "ROUGHNESS", "G1", "G2", "F")
NPAR = {1: 1, 2: 10, 3: 2}
PI = np.pi


class Exact:
    """the restatement itself: every result as NumPy gives it"""

    def __call__(self, y):
        return y

    def unit(self, y):
        """a cosine or sine"""
        return self(y)


_same = Exact()


class Nudge(Exact):
    """moves the results it is called on by one ulp: `pattern` +1 all up, -1 all down, +2 / -2 alternating by call site.  A
    cosine or sine stays within [-1, 1], as every implementation's does."""

    def __init__(self, pattern):
        self.pattern, self.n = pattern, 0

    def unit(self, y):
        return np.clip(self(y), -1.0, 1.0)

    def __call__(self, y):
        up = self.pattern > 0
        if abs(self.pattern) == 2 and self.n % 2:
            up = not up
        self.n += 1
        return np.nextafter(y, np.inf if up else -np.inf)


PATTERNS = (1, -1, 2, -2)


def fold_azimuth(azi_deg):
    """phix of :1363-1381"""
    phi = 180. - np.asarray(azi_deg, dtype=np.float64)
    return np.where(phi > 180., 180. - (phi - 180.), np.where(phi < 0., -phi, phi))


def hapke_np(params, sol, emi, azi, ulp=_same):
    """calc_Hapke_BRDF: params (10, W); sol, emi, azi broadcastable against each other -> (W,) + their shape"""
    P = np.asarray(params, dtype=np.float64)
    sol, emi, azi = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (sol, emi, azi)))
    ex = (slice(None),) + (None,) * sol.ndim
    w, K, BS0, hs, BC0, hc, RO, G1, G2, F = (P[n][ex] for n in range(10))
    i, e = sol[None], emi[None]
    phix = fold_azimuth(azi)[None]
    with np.errstate(all="ignore"):
        dark = (e >= 90.) | (i >= 90.)
        irad, erad, phirad = i / 180. * PI, e / 180. * PI, phix / 180. * PI
        mu, mu0 = ulp.unit(np.cos(erad)), ulp.unit(np.cos(irad))
        cphi = ulp.unit(np.cos(phirad))
        cg = ulp(mu * mu0 + ulp(np.sqrt(1. - mu * mu)) * ulp(np.sqrt(1. - mu0 * mu0)) * cphi)
        cg = np.where(cg > 1.0, 1.0, cg)
        cg = np.where(cg < 0.0, 0.0, cg)
        g = ulp(np.arccos(cg)) / PI * 180.
        gamma = ulp(np.sqrt(1. - w))
        r0 = (1. - gamma) / (1. + gamma)
        tb = RO * (1. - r0)
        ttb = ulp(np.tan(tb / 180. * PI))
        chi = 1. / ulp(np.sqrt(1. + PI * (ttb * ttb)))
        fphi = np.where(np.abs(phix) == 180., 0.0, ulp(np.exp(-2. * np.abs(ulp(np.tan(phix / 2. / 180. * PI))))))
        se, si = ulp.unit(np.sin(erad)), ulp.unit(np.sin(irad))
        te, ti = ulp(np.tan(erad)), ulp(np.tan(irad))

        def E12(x, tx):
            off = (tb == 0.0) | (x == 0.0)
            E1 = np.where(off, 0.0, ulp(np.exp(-2.0 / PI * 1.0 / ttb * 1. / tx)))
            E2 = np.where(off, 0.0, ulp(np.exp(-1.0 / PI * 1.0 / (ttb * ttb) * 1. / (tx * tx))))
            return E1, E2

        E1e, E2e = E12(e, te)
        E1i, E2i = E12(i, ti)
        nue = chi * (mu + se * ttb * E2e / (2.0 - E1e))
        nui = chi * (mu0 + si * ttb * E2i / (2.0 - E1i))
        ile = i <= e
        pick = lambda a, b: (np.where(ile, a, b), np.where(ile, b, a))
        (cs, cl), (ss, sl), (E1s, E1l), (E2s, E2l), (nus, _) = (pick(mu0, mu), pick(si, se), pick(E1i, E1e), pick(E2i, E2e),
                                                                pick(nui, nue))
        sh = ulp.unit(np.sin(phirad / 2.))
        sphi2 = sh * sh
        den = 2.0 - E1l - phirad / PI * E1s
        eff_s = chi * (cs + ss * ttb * (cphi * E2l + sphi2 * E2s) / den)
        eff_l = chi * (cl + sl * ttb * (E2l - sphi2 * E2s) / den)
        mu0eff, mueff = np.where(ile, eff_s, eff_l), np.where(ile, eff_l, eff_s)
        S = mueff / nue * mu0 / nui * chi / (1.0 - fphi + fphi * chi * cs / nus)
        tg = ulp(np.tan(g / 2. / 180. * PI))
        Bs = BS0 / (1. + (1. / hs) * tg)
        q = 1. / hc * tg
        Bc = BC0 / (1. + (1.3 + K) * (q + q * q))

        def H(x):
            return 1.0 / (1.0 - w * x * (r0 + (1.0 - 2.0 * r0 * x) / 2.0 * ulp(np.log((1.0 + x) / x))))

        H0e, He = H(mu0eff / K), H(mueff / K)
        cth = ulp.unit(np.cos(g / 180. * PI))
        t1 = (1. - G1 * G1) / ulp((1. - 2. * G1 * cth + G1 * G1) ** 1.5)
        t2 = (1. - G2 * G2) / ulp((1. - 2. * G2 * cth + G2 * G2) ** 1.5)
        phase = F * t1 + (1.0 - F) * t2
        r = K * w / (4. * PI) * mu0eff / (mu0eff + mueff) * (phase * (1. + Bs) + (H0e * He - 1.)) * (1. + Bc) * S
        return np.where(dark, 0.0, r / mu0)


def oren_nayar_np(params, sol, emi, azi, ulp=_same):
    """calc_OrenNayar_BRDF: params (2, W) = A, ROUGHNESS; the azimuth is taken as it comes and no angle is dark"""
    P = np.asarray(params, dtype=np.float64)
    sol, emi, azi = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (sol, emi, azi)))
    ex = (slice(None),) + (None,) * sol.ndim
    A, RO = P[0][ex], P[1][ex]
    irad, erad, phirad = sol[None] / 180. * PI, emi[None] / 180. * PI, azi[None] / 180. * PI
    sigma = RO / 180. * PI
    alpha, beta = np.maximum(irad, erad), np.minimum(irad, erad)
    s2 = sigma * sigma
    cphi = ulp.unit(np.cos(phirad))
    sa = ulp.unit(np.sin(alpha))
    b2 = 2. * beta / PI
    C1 = 1.0 - 0.5 * s2 / (s2 + 0.33)
    C2 = 0.45 * s2 / (s2 + 0.09)
    C2 = C2 * np.where(cphi >= 0, sa, sa - ulp(b2 ** 3.))
    a4 = 4. * alpha * beta / (PI * PI)
    C3 = 0.125 * s2 / (s2 + 0.09) * (a4 * a4)
    B1 = A / PI * (C1 + cphi * C2 * ulp(np.tan(beta)) + (1. - np.abs(cphi)) * C3 * ulp(np.tan((alpha + beta) / 2.)))
    B2 = 0.17 * (A * A) / PI * s2 / (s2 + 0.13) * (1.0 - cphi * (b2 * b2))
    return B1 + B2


def surface_brdf_np(lowbc, params, sol, emi, azi, ulp=_same):
    """Surface_0.calc_BRDF after its interpolation onto the wavenumbers -> (W, NTHETA)"""
    P = np.asarray(params, dtype=np.float64)
    sol = np.asarray(sol, dtype=np.float64)
    if lowbc == 1:
        return np.repeat((P[0] / PI)[:, None], sol.shape[0], axis=1)
    if lowbc == 2:
        return hapke_np(P, sol, emi, azi, ulp)
    if lowbc == 3:
        return oren_nayar_np(P, sol, emi, azi, ulp)
    raise ValueError("lowbc %r" % (lowbc,))


def matrix_tables(MU, NPHI, NF):
    """the k-only tables, in calc_brdf_matrix's own expressions: quadrature angles of MU[::-1], the azimuths k dphi in
    degrees, their fold phix, the weights wphi and cos(ic k dphi) as (NF + 1, NPHI + 1)"""
    mu = np.zeros(len(MU))
    mu[:] = np.asarray(MU, dtype=np.float64)[::-1]
    dphi = 2.0 * PI / NPHI
    k = np.arange(NPHI + 1)
    ang = np.arccos(mu) * 180.0 / PI
    azi = (k * dphi) * 180.0 / PI
    wphi = np.full(NPHI + 1, (1.0 * dphi) / (2.0 * PI))
    wphi[0] = wphi[NPHI] = (0.5 * dphi) / (2.0 * PI)
    cosk = np.cos(np.arange(NF + 1)[:, None] * (k * dphi)[None, :])
    return ang, azi, fold_azimuth(azi), wphi, cosk


def brdf_matrix_np(lowbc, params, MU, NPHI, NF, ulp=_same):
    """ForwardModel_0.calc_brdf_matrix after the interpolation of the parameters -> (W, NMU, NMU, NF + 1)"""
    P = np.atleast_2d(np.asarray(params, dtype=np.float64))
    W, NMU = P.shape[1], len(MU)
    out = np.zeros((W, NMU, NMU, NF + 1))
    if lowbc == 1:
        out[:, :, :, 0] = (P[0] / PI)[:, None, None]
    if lowbc != 2:
        return out
    ang, azi, _, wphi, cosk = matrix_tables(MU, NPHI, NF)
    # B[w, j, i, k]: j the solar angle, i the emission angle
    B = hapke_np(P, ang[:, None, None], ang[None, :, None], azi[None, None, :], ulp)
    acc = np.zeros((W, NMU, NMU, NF + 1))                      # [w, j, i, ic]
    for k in range(NPHI + 1):
        acc += (wphi[k] * B[:, :, :, k])[..., None] * cosk[None, None, None, :, k]
    return np.ascontiguousarray(np.transpose(acc, (0, 2, 1, 3)))


# ---- cases ------------------------------------------------------------------------------------------------------------
def hapke_params(rng, W, h):
    """W plausible Hapke parameter sets; the opposition widths hs, hc drawn around h"""
    P = np.empty((10, W))
    P[0] = rng.uniform(0.2, 0.9, W); P[1] = rng.uniform(1.0, 1.4, W); P[2] = rng.uniform(0.2, 1.0, W)
    P[3] = h * rng.uniform(1.0, 1.6, W); P[4] = rng.uniform(0.1, 0.8, W); P[5] = h * rng.uniform(1.0, 1.6, W)
    P[6] = rng.uniform(5.0, 25.0, W); P[7] = rng.uniform(-0.5, -0.1, W); P[8] = rng.uniform(0.1, 0.6, W)
    P[9] = rng.uniform(0.2, 0.8, W)
    return P


def _edge_triples(opposition):
    """(sol, emi, azi) rows that reach every branch of the point function; azimuth 180 is the opposition direction"""
    t = [(20., 50., 30.), (50., 20., 30.), (35., 35., 75.),            # i < e, i > e, i == e
         (40., 0., 10.), (0., 40., 10.), (0., 1e-3, 0.),               # e = 0, i = 0, next to both
         (40., 90., 10.), (95., 40., 10.), (90., 95., 180.),           # dark
         (25., 45., 0.), (25., 45., 360.), (25., 45., 200.), (25., 45., 359.9), (45., 25., 0.),
         (60., 60., 0.),                                               # cg < 0 before the clamp
         (10., 80., 120.), (80., 10., 120.), (89.9, 89.9, 90.), (1e-3, 30., 45.)]
    if opposition:
        t += [(30., 30., 180.), (25., 45., 180.), (0., 0., 180.), (0., 0., 0.), (70., 70., 180.)]   # i = e = 0 is opposition too
    else:
        t += [(30., 31., 180.), (25., 45., 180.), (30., 30., 178.), (70., 70., 170.)]
    return t


def _triples(rng, n, opposition):
    t = _edge_triples(opposition)
    while len(t) < n:
        i, e = rng.uniform(0.5, 89.0, 2)
        t.append((round(float(i), 3), round(float(e), 3), round(float(rng.uniform(0.0, 360.0)), 3)))
    a = np.array(t[:n])
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def gauss_mu(nmu):
    """quadrature cosines as Scatter_0 stores them: ascending, the last one near 1"""
    x, _ = np.polynomial.legendre.leggauss(nmu)
    return 0.5 * (x + 1.0)


POINT_CASES = ("hapke-opposition", "hapke-narrow", "oren-nayar", "lambert")
MATRIX_SHAPES = {"m-5-101-2": (5, 101, 2, 3), "m-5-100-0": (5, 100, 0, 3), "m-7-101-4": (7, 101, 4, 3),
                 "m-16-101-8": (16, 101, 8, 3), "m-16-100-2": (16, 100, 2, 3), "m-5-101-2-w70": (5, 101, 2, 70)}
MATRIX_CASES = tuple(MATRIX_SHAPES) + ("m-lambert", "m-oren-nayar")
NTHETA = 70


def golden_cases():
    """name -> dict(kind 'points' | 'matrix', lowbc, params, and the angles or MU / NPHI / NF)"""
    cases = {}
    rng = np.random.default_rng(20260118)
    # array level: W = 3, NTHETA = 70 (more than one wavefront); wavenumber 1 has no roughness, wavenumber 2 w = 0.999
    for name, h, opp in (("hapke-opposition", 0.6, True), ("hapke-narrow", 0.05, False)):
        P = hapke_params(rng, 3, h)
        P[6, 1] = 0.0
        P[0, 2] = 0.999
        sol, emi, azi = _triples(rng, NTHETA, opp)
        cases[name] = dict(kind="points", lowbc=2, params=P, sol=sol, emi=emi, azi=azi)
    sol, emi, azi = _triples(rng, NTHETA, True)                       # cos(azi) of both signs, dark angles are not special
    cases["oren-nayar"] = dict(kind="points", lowbc=3, params=np.array([[0.3, 0.7, 0.5], [20.0, 0.0, 35.0]]),
                               sol=sol, emi=emi, azi=azi)
    cases["lambert"] = dict(kind="points", lowbc=1, params=np.array([[0.0, 0.25, 1.0]]), sol=sol, emi=emi, azi=azi)
    # matrices: an even NPHI puts azimuth 180 -- exact opposition on the diagonal -- among the nodes, so hs, hc >= 0.5
    for name, (nmu, nphi, nf, W) in MATRIX_SHAPES.items():
        P = hapke_params(rng, W, 0.6)
        P[6, 1] = 0.0
        P[0, 2] = 0.999
        cases[name] = dict(kind="matrix", lowbc=2, params=P, MU=gauss_mu(nmu), NPHI=nphi, NF=nf)
    cases["m-lambert"] = dict(kind="matrix", lowbc=1, params=np.array([[0.0, 0.25, 1.0]]), MU=gauss_mu(5), NPHI=101, NF=2)
    cases["m-oren-nayar"] = dict(kind="matrix", lowbc=3, params=np.array([[0.3, 0.7, 0.5], [20.0, 0.0, 35.0]]),
                                 MU=gauss_mu(5), NPHI=101, NF=2)
    assert tuple(cases) == POINT_CASES + MATRIX_CASES
    return cases


INPUTS = {"points": ("lowbc", "params", "sol", "emi", "azi"), "matrix": ("lowbc", "params", "MU", "NPHI", "NF")}


def evaluate_np(d, ulp=_same):
    if d["kind"] == "points":
        return surface_brdf_np(int(d["lowbc"]), d["params"], d["sol"], d["emi"], d["azi"], ulp)
    return brdf_matrix_np(int(d["lowbc"]), d["params"], d["MU"], int(d["NPHI"]), int(d["NF"]), ulp)


def deviation(got, ref):
    """largest |got - ref| relative to the row maximum (points: per wavenumber; matrix: per plane [w, :, :, ic]); rows that
    are zero in the reference must be zero"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    axes = (1,) if ref.ndim == 2 else (1, 2)
    top = np.max(np.abs(ref), axis=axes, keepdims=True)
    err = np.abs(got - ref)
    if np.any((top == 0) & (np.max(err, axis=axes, keepdims=True) > 0)) or not np.all(np.isfinite(got)):
        return np.inf
    return float(np.max(err / np.where(top == 0, 1.0, top)))


def load_golden(path):
    z = np.load(path)
    out = {}
    for key in z.files:
        name, field = key.split("__")
        out.setdefault(name, {})[field] = z[key]
    for d in out.values():
        d["kind"] = str(d["kind"])
    return out
