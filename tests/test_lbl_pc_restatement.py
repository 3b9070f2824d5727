"""The NumPy restatement of the pseudo-continuum (tests/lbl_pc_cases.py: every sum gathered by its owner, as the kernels
do) against the reference's results in tests/golden/lbl_pseudo_continuum.npz (tools/golden/gen_golden_lbl_pc.py), bit for
bit: this pins the checker the GPU tests use at sizes the reference does not reach, and the claim that the gather form needs
no other summation order than the reference's."""
import os

import numpy as np
import pytest

import lbl_pc_cases as pc

CASES = ("regular", "jittered", "overlapping", "ends_inside", "starts_inside", "fine_bins", "lorentz", "gaussian",
         "one_neighbour", "onto_nonzero", "two_broadeners", "three_broadeners")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return pc.load_golden(os.path.join(golden_dir, "lbl_pseudo_continuum.npz"))


def test_fixture_holds_the_cases_and_is_what_the_generator_builds(golden):
    assert sorted(golden) == sorted(CASES)
    built = pc.golden_cases()
    for name in CASES:
        for k in pc.INPUTS:
            assert np.array_equal(np.asarray(built[name][k]), np.asarray(golden[name][k])), (name, k)


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_bit_for_bit(golden, name):
    g = golden[name]
    out = g["out0"].copy()
    store, x = pc.pseudo_continuum_np(*pc.engine_args(g), out, n_neighbour_bins=g["n_neighbour_bins"])
    assert np.array_equal(store, g["store"])
    assert np.array_equal(x, g["store_x"])
    assert np.array_equal(out, g["out"])
    changed = np.count_nonzero(g["out"] - g["out0"])
    if name in pc.COVERING:
        assert changed >= out.size - 1            # a restatement that adds nothing cannot pass
    if name == "starts_inside":
        assert changed == 0 and not np.any(g["store_x"])


def test_window_of_the_restatement_equals_the_whole(golden):
    g = golden["jittered"]
    whole, part = g["out0"].copy(), g["out0"].copy()
    pc.pseudo_continuum_np(*pc.engine_args(g), whole, n_neighbour_bins=3)
    pc.pseudo_continuum_np(*pc.engine_args(g), part, n_neighbour_bins=3, j_from=300, j_to=420)
    assert np.array_equal(part[300:420], whole[300:420]) and not np.any(part[:300]) and not np.any(part[420:])
