"""ansfm_mie_makephase on the GPU (Scatter_0.makephase for iscat 1 .. 4) against the reference's results in
tests/golden/mie.npz: radius counts exactly; cross-sections and phase function within 100 x the deviation the NumPy
restatement shows with the kernels' summation order (tests/test_mie_host.py) -- the order alone costs that much, the
factor covers a few ulp per term from the device's sin / cos / exp / log / pow -- and never above the project's parity bar
of 1e-6.  Then bit-identity across radius blocks, and the clean errors (return codes; nothing is provoked on the device).

Measured on MI355X: see the table there."""
import os

import numpy as np
import pytest

import mie_cases as mc
from test_mie_host import CHUNK_ORDER_DEVIATION

pytestmark = pytest.mark.gpu

CASES = tuple(mc.golden_cases())
BOUNDS = tuple(min(100.0 * d, 1e-6) for d in CHUNK_ORDER_DEVIATION)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return mc.load_golden(os.path.join(golden_dir, "mie.npz"))


@pytest.fixture(scope="module")
def engine():
    from archnemesis_dist_amd.engine import AnsfmEngine
    eng = AnsfmEngine(0)
    yield eng
    eng.close()


def _run(engine, g, **kw):
    return engine.mie_makephase(g["wavel"], int(g["iscat"]), g["dsize"], g["rs"], g["refindx"], g["theta"], return_counts=True, **kw)


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(engine, golden, name):
    g = golden[name]
    xs, xe, thetax, ph, counts = _run(engine, g)
    dev = mc.deviations((xs, xe, ph), g)
    print("%s: radii %s  cross-sections %.2e  phase / max %.2e  phase pointwise %.2e  (bounds %.1e %.1e %.1e)" %
          ((name, list(counts)) + dev + BOUNDS))
    assert np.array_equal(counts, g["n_radii"])
    assert np.array_equal(thetax, g["thetax"])
    assert all(d <= b for d, b in zip(dev, BOUNDS)), dev


@pytest.mark.parametrize("name", ["lognormal-open-90", "closed-64", "closed-65"])
def test_radius_block_changes_no_bit(engine, golden, name):
    g = golden[name]
    ref = _run(engine, g)
    for block in (64, 128):
        got = _run(engine, g, radius_block=block)
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), (name, block)
    if name == "lognormal-open-90":      # the wavelengths end in different blocks of 64 radii (177, 199 and 234 radii)
        assert len(set(int(c - 1) // 64 for c in ref[4])) > 1


def test_clean_errors(engine, golden):
    g = golden["lognormal-open-90"]
    with pytest.raises(ValueError, match="outside"):
        engine.mie_makephase(g["wavel"], 2, g["dsize"], g["rs"], g["refindx"], [0.0, 95.0])
    with pytest.raises(ValueError, match="iscat"):
        engine.mie_makephase(g["wavel"], 6, g["dsize"], g["rs"], g["refindx"], g["theta"])
    # x = 201, m = 1.05: the series needs more than nmx2 = int(1.05 x) = 211 terms; the reference fails there too (TypeError)
    with pytest.raises(ValueError, match=r"radius 16 um"):
        engine.mie_makephase([0.5], 4, [16.0, 0.0, 0.0], [16.0, 16.0, 16.0], [[1.05, 0.0]], [0.0, 90.0])
    with pytest.raises(ValueError, match="did not terminate"):
        engine.mie_makephase(g["wavel"], 2, g["dsize"], g["rs"], g["refindx"], g["theta"], radius_cap=128)
    # ... and the engine still answers
    xs = _run(engine, golden["closed-even"])[0]
    assert abs(xs[0] / golden["closed-even"]["xscat"][0] - 1) < 1e-6
