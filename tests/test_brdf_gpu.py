"""ansfm_surface_brdf and ansfm_brdf_matrix on the GPU against the reference's results in tests/golden/brdf.npz.

Every case within its own bound: 16 x the deviation the NumPy restatement shows when cg and the result of every
cos / sin / tan / exp / log / arccos / sqrt / pow are moved by one ulp (stored per case by tools/golden/gen_golden_brdf.py,
relative to the row -- matrix: plane -- maximum; never above the parity bar of 1e-6, tests/test_brdf_host.py).  Then what must
hold bit for bit: a matrix does not depend on which wavenumbers share a call, nor a Fourier plane on how many are asked
for; a dark angle gives exactly 0.  The clean errors (return codes; nothing is provoked on the device).  And end to end:
scloud11wave_core with lowbc = 2 on the engine's matrix against the same call on the golden matrix.

The bounds and the deviations measured on MI355X are tabulated in DESIGN.md 4.5f."""
import os

import numpy as np
import pytest

import brdf_cases as bc

pytestmark = pytest.mark.gpu

CASES = bc.POINT_CASES + bc.MATRIX_CASES


@pytest.fixture(scope="module")
def golden(golden_dir):
    return bc.load_golden(os.path.join(golden_dir, "brdf.npz"))


@pytest.fixture(scope="module")
def engine():
    from archnemesis_dist_amd.engine import AnsfmEngine
    eng = AnsfmEngine(0)
    yield eng
    eng.close()


def _run(engine, g, params=None, NF=None):
    P = g["params"] if params is None else params
    if g["kind"] == "points":
        return engine.surface_brdf(int(g["lowbc"]), P, g["sol"], g["emi"], g["azi"])
    return engine.brdf_matrix(int(g["lowbc"]), P, g["MU"], int(g["NPHI"]), int(g["NF"]) if NF is None else NF)


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(engine, golden, name):
    g = golden[name]
    got = _run(engine, g)
    dev, bound = bc.deviation(got, g["ref"]), 16.0 * float(g["ulp"])
    print("%s: deviation / row maximum %.2e  (bound %.2e, one ulp %.2e)" % (name, dev, bound, float(g["ulp"])))
    assert got.shape == g["ref"].shape
    assert dev <= bound


def test_wavenumber_slices_change_no_bit(engine, golden):
    g = golden["m-5-101-2-w70"]
    whole = _run(engine, g)
    parts = [_run(engine, g, params=np.ascontiguousarray(g["params"][:, s])) for s in (slice(0, 3), slice(3, 70))]
    assert np.array_equal(whole, np.concatenate(parts, axis=0))


def test_fourier_planes_do_not_depend_on_nf(engine, golden):
    g = golden["m-5-101-2"]
    assert np.array_equal(_run(engine, g), _run(engine, g, NF=8)[..., :3])


def test_dark_angles_are_exactly_zero(engine, golden):
    g = golden["hapke-opposition"]
    got = _run(engine, g)
    dark = (g["sol"] >= 90.) | (g["emi"] >= 90.)
    assert np.count_nonzero(dark) >= 3
    assert np.all(got[:, dark] == 0.0) and np.all(got[:, ~dark] > 0.0)


def test_clean_errors(engine, golden):
    g = golden["m-5-101-2"]
    P, MU = g["params"], g["MU"]
    with pytest.raises(ValueError, match="lowbc"):
        engine.brdf_matrix(4, P, MU, 101, 2)
    with pytest.raises(ValueError, match="lowbc"):
        engine.surface_brdf(0, P, [10.], [20.], [30.])
    with pytest.raises(ValueError, match="nmu"):
        engine.brdf_matrix(2, P, [], 101, 2)
    with pytest.raises(ValueError, match="nphi"):
        engine.brdf_matrix(2, P, MU, 0, 2)
    with pytest.raises(ValueError, match="nf"):
        engine.brdf_matrix(2, P, MU, 101, 33)
    with pytest.raises(ValueError, match="params"):
        engine.brdf_matrix(2, P[:9], MU, 101, 2)
    with pytest.raises(ValueError, match="one length"):
        engine.surface_brdf(2, P, [10., 20.], [20.], [30., 40.])
    # the C entry checks what the engine method cannot get wrong: a phix table that is not the fold of its azimuths
    import ctypes as C
    ang, azi, phix, wphi, cosk = engine.brdf_tables(MU, 101, 2)
    out = np.empty((P.shape[1], 5, 5, 3))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = phix.copy(); bad[7] += 1.0
    Pc = np.ascontiguousarray(P)
    assert engine._lib.ansfm_brdf_matrix(engine._ctx, 2, P.shape[1], ptr(Pc), 5, ptr(ang), 101, 2, ptr(azi), ptr(bad), ptr(wphi),
                                         ptr(cosk), ptr(out)) == 1
    assert engine._lib.ansfm_brdf_matrix(engine._ctx, 2, P.shape[1], ptr(Pc), 5, ptr(ang), 101, 2, ptr(azi), ptr(phix), None,
                                         ptr(cosk), ptr(out)) == 1
    # ... and the engine still answers
    assert bc.deviation(_run(engine, g), g["ref"]) <= 16.0 * float(g["ulp"])
    assert not np.any(engine.brdf_matrix(0, np.zeros((1, 3)), MU, 101, 2)) and not np.any(engine.brdf_matrix(3, P[:2], MU, 101, 2))


def test_scattering_core_on_the_engines_matrix(engine, golden):
    """The matrix enters the surface operator linearly (Multiple_Scattering_Core.py:828): one atmosphere over a Hapke surface,
    the spectrum from the engine's matrix within 1e-9 of the spectrum's maximum of the one from the golden matrix."""
    g = golden["m-5-101-2"]
    nmu, nf, nphi, W = 5, int(g["NF"]), int(g["NPHI"]), g["params"].shape[1]
    x, wt = np.polynomial.legendre.leggauss(nmu)
    assert np.array_equal(0.5 * (x + 1.0), g["MU"])
    mu1, wt1 = g["MU"], 0.5 * wt
    nlay, ng, ncont, nth = 4, 1, 1, 3
    phasarr = np.zeros((ncont, W, 2, nth))
    phasarr[0, :, 0, :3] = [0.7, 0.6, -0.3]                       # Henyey-Greenstein f, g1, g2 (imie = 0)
    phasarr[0, :, 1, :] = [-1.0, 0.0, 1.0]
    taus = np.full((W, ng, nlay), 0.05); omegas = np.full((W, ng, nlay), 0.6)
    tauray = np.zeros((W, nlay)); lfrac = np.ones((W, ncont, nlay))
    bnu = np.zeros((W, nlay)); radg = np.zeros((W, nmu)); solar = np.full(W, 1.0)
    args = lambda brdf: ([phasarr, radg, [35.0], [20.0], solar, [60.0], 2, brdf, mu1, wt1, nf, np.arange(W, dtype=float), bnu, taus,
                          tauray, omegas, nphi, 0, 0, lfrac])
    ref = engine.scloud11wave_core(*args(g["ref"]))
    got = engine.scloud11wave_core(*args(_run(engine, g)))
    assert ref.shape == (1, ng, W) and np.all(ref > 0)
    assert np.max(np.abs(got - ref)) <= 1e-9 * np.max(np.abs(ref))
    dark = engine.scloud11wave_core(*args(np.zeros_like(g["ref"])))
    assert np.max(np.abs(dark - ref)) > 1e-3 * np.max(np.abs(ref))     # the surface is seen through this atmosphere
