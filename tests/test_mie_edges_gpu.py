"""ansfm_mie_makephase on the GPU at the edges the eight golden cases leave out (tests/mie_cases.py::edge_cases) against the
reference's results in tests/golden/mie_edges.npz: a refractive index per wavelength, the block of radii halved by the 1 GiB
workspace bound, a failing series behind the cut-off of an open range, nmx1 around its switch at 150, x = 2011, strong
absorption, x down to 3e-3, 1 and 33 angles, 130 wavelengths, a closed range of 2 radii, and open ranges that end on the last
radius of a chunk or block and on the first radius of the next.

Bounds per case and measure: min(1e-6, 100 x EDGE_DEVIATION[name]) (tests/test_mie_host.py), the larger of what the kernels'
order of the sum costs and of what one ulp in sin, cos, exp, log and pow moves -- both measured on the host against the
reference, never on the kernels.  The bit-identity tests rest on the reduction order depending on the radius index alone.

Measured on MI355X: see the table there."""
import os

import numpy as np
import pytest

import mie_cases as mc
from test_mie_host import EDGE_DEVIATION

pytestmark = pytest.mark.gpu

CASES = tuple(mc.edge_cases())


@pytest.fixture(scope="module")
def golden(golden_dir):
    return mc.load_golden(os.path.join(golden_dir, "mie_edges.npz"))


@pytest.fixture(scope="module")
def engine():
    from archnemesis_dist_amd.engine import AnsfmEngine
    eng = AnsfmEngine(0)
    yield eng
    eng.close()


def _run(engine, g, waves=slice(None), theta=None, rs=None, **kw):
    return engine.mie_makephase(g["wavel"][waves], int(g["iscat"]), g["dsize"], g["rs"] if rs is None else rs, g["refindx"][waves],
                                g["theta"] if theta is None else theta, return_counts=True, **kw)


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


@pytest.mark.parametrize("name", CASES)
def test_edge_cases(engine, golden, name):
    g = golden[name]
    bounds = tuple(min(100.0 * d, 1e-6) for d in EDGE_DEVIATION[name])
    xs, xe, thetax, ph, counts = _run(engine, g)
    dev = mc.deviations((xs, xe, ph), g)
    print("%s: radii %s  cross-sections %.2e  phase / max %.2e  phase pointwise %.2e  (bounds %.1e %.1e %.1e)" %
          ((name, counts.tolist() if counts.shape[0] <= 4 else "%d x %s" % (counts.shape[0], set(counts.tolist()))) + dev + bounds))
    assert np.array_equal(counts, g["n_radii"])
    assert np.array_equal(thetax, g["thetax"])
    assert ph.shape == g["phas"].shape == (g["wavel"].shape[0], mc.nphas_of(g["theta"]))
    assert all(d <= b for d, b in zip(dev, bounds)), dev


@pytest.mark.parametrize("name", ["perwave-m", "waves-130"])
def test_each_wavelength_reads_its_own_index(engine, golden, name):
    g = golden[name]
    assert len(set(map(tuple, g["refindx"]))) == g["wavel"].shape[0]
    joint = _run(engine, g)
    for i in range(g["wavel"].shape[0]):
        alone = _run(engine, g, waves=slice(i, i + 1))
        for a, b in zip((alone[0], alone[1], alone[3], alone[4]), (joint[0], joint[1], joint[3], joint[4])):
            assert np.array_equal(a[0], b[i]), (name, i)


def test_failure_behind_the_cutoff_does_not_count(engine, golden):
    g = golden["fail-behind-cut"]
    counts = _run(engine, g)[4]
    assert list(counts) == [26]
    # the same radii as a closed range up to index 93, the first whose series needs more than nmx2 terms (a return code)
    rs = np.array([g["rs"][0], g["rs"][0] + (93 + 0.25) * g["rs"][2], g["rs"][2]])
    assert mc.radius_count(rs) == 94
    with pytest.raises(ValueError, match=r"radius 9\.4 um \(index 93\)"):
        _run(engine, g, rs=rs)
    assert list(_run(engine, g)[4]) == [26]


def test_halved_block_changes_no_bit(engine, golden):
    g = golden["ws-halved"]
    ref = _run(engine, g)
    ms, blocks, block_radii = engine.mie_last()
    print("ws-halved: %d blocks of at most %d radii, kernels %.1f ms" % (blocks, block_radii, ms))
    assert blocks >= 2 and block_radii < 512
    for block in (64, 128):
        _same_bits(ref, _run(engine, g, radius_block=block), block)
        assert engine.mie_last()[2] == block


@pytest.mark.parametrize("name", tuple(mc.OPEN_STEPS))
def test_open_range_ends_at_a_chunk_boundary(engine, golden, name):
    g = golden[name]
    ref = _run(engine, g)
    assert list(ref[4]) == [mc.EDGE_EXPECTED_RADII[name]] == [int(name.split("-")[1])]
    _same_bits(ref, _run(engine, g, radius_block=64), name)


def test_theta_shapes(engine, golden):
    for name, nphas in (("theta-0", 2), ("theta-90", 1), ("theta-33", 66), ("theta-33-90", 65)):
        xs, xe, thetax, ph, counts = _run(engine, golden[name])
        assert xs.shape == xe.shape == (1,) and thetax.shape == (nphas,) and ph.shape == (1, nphas), name
    a, b = _run(engine, golden["theta-33"]), _run(engine, golden["theta-33-90"])
    assert np.array_equal(golden["theta-33"]["theta"][:32], golden["theta-33-90"]["theta"][:32])
    # the 32 angles the two share, and their mirror images: thetax = (t0 .. t31, t32 | 90, 180 - ...)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[3][:, :32], b[3][:, :32]) and np.array_equal(a[2][:32], b[2][:32])
    assert np.array_equal(a[3][:, 34:], b[3][:, 33:]) and np.array_equal(a[2][34:], b[2][33:])
