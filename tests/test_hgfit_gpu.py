"""ansfm_hg_fit on the GPU (Scatter_0.subfithgm) against the reference's results in tests/golden/hgfit.npz.  Per case and
per measure -- (f, g1, g2) and rms, relative -- the bound is min(1e-6, 100 x HGFIT_DEVIATION[case]) (tests/test_hgfit_host.py):
what the kernel's order of the sums, its elimination and one ulp in cos, log and pow cost on the host, against the reference,
times the project's factor for a few ulp per transcendental from the device; never measured on the kernel.  The fit is
defined to about 1e-8 by its own stopping rule and one ulp can move an accept / reject decision, so call counts are printed,
not asserted.  Then: a fit alone gives the bits it has in a joint call, a repeated call the same bits, and the clean errors
(return codes; nothing is provoked on the device).

Measured on MI355X: see the table there."""
import ctypes as C
import os

import numpy as np
import pytest

import hgfit_cases as hc
from test_hgfit_host import HGFIT_DEVIATION

pytestmark = pytest.mark.gpu

CASES = hc.CASE_NAMES
BOUNDS = {name: tuple(min(1e-6, 100.0 * d) for d in dev) for name, dev in HGFIT_DEVIATION.items()}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return hc.load_golden(os.path.join(golden_dir, "hgfit.npz"))


@pytest.fixture(scope="module")
def engine():
    from archnemesis_dist_amd.engine import AnsfmEngine
    eng = AnsfmEngine(0)
    yield eng
    eng.close()


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(engine, golden, name):
    g = golden[name]
    got = engine.hg_fit(g["theta"], g["phase"], return_counts=True)
    dev = hc.deviations(got, (g["f"], g["g1"], g["g2"], g["rms"]))
    c, rc = got[4], g["counts"]
    print("%s: (f, g1, g2) %.2e  rms %.2e  (bounds %.1e %.1e)  calls %d .. %d (reference %d .. %d)  accepted %d .. %d (%d .. %d)  "
          "kernel %.3f ms" % ((name,) + dev + BOUNDS[name] + (c[:, 0].min(), c[:, 0].max(), rc[:, 0].min(), rc[:, 0].max(),
                                                             c[:, 1].min(), c[:, 1].max(), rc[:, 1].min(), rc[:, 1].max(),
                                                             engine.hg_fit_last())))
    assert c.dtype == np.int32 and c.shape == rc.shape
    assert all(d <= b for d, b in zip(dev, BOUNDS[name])), (dev, BOUNDS[name])
    if name == "zero-phase":            # equal special values: the start point, rms = inf, no call accepted
        assert (got[0][0], got[1][0], got[2][0]) == (0.5, 0.5, -0.5) and np.isposinf(got[3][0]) and list(c[0]) == [hc.NOVER, 0]


def test_gamma_6_uses_all_calls(engine, golden):
    g = golden["gamma-6"]
    counts = engine.hg_fit(g["theta"], g["phase"], return_counts=True)[4]
    assert counts[:, 0].max() == hc.NOVER and np.all(counts[:, 1] <= counts[:, 0]) and np.all(counts[:, 0] >= 1)


@pytest.mark.parametrize("name", ["lognormal-41", "fits-130"])
def test_a_fit_alone_gives_the_bits_of_the_joint_call(engine, golden, name):
    g = golden[name]
    joint = engine.hg_fit(g["theta"], g["phase"], return_counts=True)
    rows = range(g["phase"].shape[0]) if name == "lognormal-41" else (0, 3, 4, 63, 64, 127, 128, 129)
    for i in rows:
        alone = engine.hg_fit(g["theta"], g["phase"][i:i + 1], return_counts=True)
        for a, b in zip(alone, joint):
            assert np.array_equal(a[0], b[i]), (name, i)


def test_a_repeated_call_gives_the_same_bits(engine, golden):
    g = golden["nphase-129"]
    first = engine.hg_fit(g["theta"], g["phase"], return_counts=True)
    engine.hg_fit(golden["gamma-6"]["theta"], golden["gamma-6"]["phase"])       # another shape in between
    again = engine.hg_fit(g["theta"], g["phase"], return_counts=True)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)


def test_clean_errors(engine, golden):
    g = golden["lognormal-41"]
    with pytest.raises(ValueError, match="0 angles"):
        engine.hg_fit(np.zeros(0), np.zeros((2, 0)))
    n = engine.HG_FIT_NPHASE_CAP + 1
    with pytest.raises(ValueError, match="%d angles" % n):
        engine.hg_fit(np.linspace(0.0, 180.0, n), np.ones((1, n)))
    with pytest.raises(ValueError, match="theta"):
        engine.hg_fit(g["theta"][:-1], g["phase"])
    # a null pointer, by return code
    out = [np.empty(4) for _ in range(4)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    theta, phase = np.ascontiguousarray(g["theta"]), np.ascontiguousarray(g["phase"])
    lib, ctx = engine._lib, engine._ctx
    assert lib.ansfm_hg_fit(ctx, 4, 41, None, ptr(phase), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), None) == 1
    assert lib.ansfm_hg_fit(ctx, 4, 41, ptr(theta), ptr(phase), ptr(out[0]), ptr(out[1]), ptr(out[2]), None, None) == 1
    assert b"null pointer" in lib.ansfm_last_error(ctx)
    assert lib.ansfm_hg_fit(ctx, 0, 41, ptr(theta), ptr(phase), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), None) == 1
    # a singular fit is named (alpha does not depend on the phase function, so every fit at this one angle is singular and
    # the first is reported): the reference ends in "Singular matrix" there
    s = golden["singular-90"]
    with pytest.raises(ValueError, match="fit 0:.*zero pivot"):
        engine.hg_fit(s["theta"], np.concatenate([s["phase"], 2.0 * s["phase"]], axis=0))
    # ... and the engine still answers; counts may be left out
    assert lib.ansfm_hg_fit(ctx, 4, 41, ptr(theta), ptr(phase), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), None) == 0
    dev = hc.deviations(out, (g["f"], g["g1"], g["g2"], g["rms"]))
    assert all(d <= b for d, b in zip(dev, BOUNDS["lognormal-41"])), dev
