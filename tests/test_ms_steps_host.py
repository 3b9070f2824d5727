"""CPU-only: the steps the three multiple-scattering chain kernels share (csrc/ansfm_ms_chain_steps.h), run by
tests/host/ms_steps_main.cpp, which is built with the host compiler under AddressSanitizer and UBSan and run as a child process.
The expectations are written out by hand from Multiple_Scattering_Core.scloud11wave_core (:846-860 the layer's scalars, :321-340
the doubling start, :903-945 the brackets in the quadrature, :945-958 the Fourier sum) in numbers that are exact in binary, or
computed with NumPy in the reference's order."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "archnemesis_dist_amd", "csrc")
EMPTY, ABSORBING, SCATTERING = 0, 1, 2

MU5 = [0.95, 0.77, 0.5, 0.23, 0.05]                        # a descending 5-point quadrature
MU7 = [0.97, 0.87, 0.70, 0.5, 0.30, 0.13, 0.03]            # 7 points in 16 slots: the padding is mu = 1 (MsParams::nmu_real)
MU7_PADDED = MU7 + [1.0] * 9

# name, step, arguments
CASES = [
    # five layers' worth of scalars: taut, omega as given, tauray
    ("omega_below_0", "scalars", [2.0, -0.5, 0.25]),       # clamped to 0: tauscat = 0 - 0.25 -> 0, omega = 0.25 / 2
    ("omega_above_1", "scalars", [2.0, 1.5, 0.5]),         # clamped to 1: tauscat = 2 - 0.5, omega = (1.5 + 0.5) / 2
    ("taur_above_scat", "scalars", [1.0, 0.25, 0.5]),      # tauscat = 0.25 - 0.5 -> 0, omega = 0.5
    ("taut_0", "scalars", [0.0, 0.5, 0.0]),                # empty: omega = 0 / 0 is never read
    ("omega_0", "scalars", [3.0, 0.0, 0.0]),               # absorbing only
    # log2(taut) + 12 = -0.5, 0.5, 11.9: int() truncates toward zero (floor would give -1 in the first); order 0 and order 2
    ("nd_m0p5", "doubling", [2.0 ** -12.5, 0.75, 0.5, 0.25, 0]),
    ("nd_0p5", "doubling", [2.0 ** -11.5, 0.75, 0.5, 0.25, 2]),
    ("nd_11p9", "doubling", [2.0 ** -0.1, 0.75, 0.5, 0.25, 0]),
    # nq, z, the slots
    ("z_on_point", "bracket", [5, 0.5] + MU5),             # mu[2] >= z > mu[3]
    ("z_on_last_point", "bracket", [5, 0.05] + MU5),
    ("z_below_last", "bracket", [5, 0.01] + MU5),
    ("z_above_first", "bracket", [5, 0.99] + MU5),
    ("z_inside", "bracket", [5, 0.3] + MU5),
    ("padded_inside", "bracket", [7, 0.6] + MU7_PADDED),
    ("padded_below_last", "bracket", [7, 0.01] + MU7_PADDED),   # the last REAL interval, not slot 14
    ("padded_above_first", "bracket", [7, 0.99] + MU7_PADDED),
    # yx[0..3], t, u
    ("bilinear", "bilinear", [1.0, 2.0, 4.0, 8.0, 0.25, 0.5]),
    # the terms of a path's azimuth series
    ("two_small_terms", "fourier", [1.0, 1e-7, 1e-8, 5.0]),     # stops after the second small term; 5.0 is never added
    ("one_small_term", "fourier", [1.0, 1e-7, 0.5, 1e-9, 0.25]),   # a small term, a large one, a small one: no two in a row
]


def _compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ms_steps") / "ms_steps_main")
    # the sanitizers' runtimes inside the program (clang's default): it then starts whatever else the loader brings in first
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all"] + static + ["-I", CSRC, os.path.join(ROOT, "tests", "host", "ms_steps_main.cpp"), "-o", exe],
                   check=True, timeout=300)
    text = "".join("%s %s %s\n" % (name, step, " ".join(float(a).hex() if step != "bracket" or i > 0 else str(int(a))
                                                         for i, a in enumerate(args))) for name, step, args in CASES)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        name, *fields = line.split()
        out[name] = {k: (int(v) if k in ("kind", "nd", "bracket", "terms") else float.fromhex(v)) for k, v in (f.split("=") for f in fields)}
    return out


def test_layer_scalars(steps):
    assert steps["omega_below_0"] == dict(tauscat=0.0, omega=0.125, kind=SCATTERING)
    assert steps["omega_above_1"] == dict(tauscat=1.5, omega=1.0, kind=SCATTERING)
    assert steps["taur_above_scat"] == dict(tauscat=0.0, omega=0.5, kind=SCATTERING)
    assert steps["taut_0"]["kind"] == EMPTY and steps["taut_0"]["tauscat"] == 0.0
    assert steps["omega_0"] == dict(tauscat=0.0, omega=0.0, kind=ABSORBING)


@pytest.mark.parametrize("name,nd", [("nd_m0p5", 0), ("nd_0p5", 0), ("nd_11p9", 11)])
def test_doubling_start(steps, name, nd):
    taut, omega, tauscat, taur, ic = next(a for n, _, a in CASES if n == name)
    got = steps[name]
    assert got["nd"] == nd == int(np.log2(taut) + 12)
    assert got["tau0"] == (taut / 2.0 ** nd if nd >= 1 else taut)
    assert got["con"] == omega * math.pi * (2.0 if ic == 0 else 1.0)
    assert got["fr"] == taur / (tauscat + taur) and got["fs"] == tauscat / (tauscat + taur)


@pytest.mark.parametrize("name,want", [("z_on_point", 2), ("z_on_last_point", 3), ("z_below_last", 3), ("z_above_first", 0),
                                       ("z_inside", 2), ("padded_inside", 2), ("padded_below_last", 5), ("padded_above_first", 0)])
def test_bracket(steps, name, want):
    assert steps[name]["bracket"] == want


def test_bilinear(steps):
    # (1 - t)(1 - u) yx0 + t (1 - u) yx1 + t u yx3 + (1 - t) u yx2 = 0.375 + 0.25 + 1 + 1.5
    assert steps["bilinear"]["value"] == 3.125


def test_fourier_break(steps):
    assert steps["two_small_terms"] == dict(rad=(1.0 + 1e-7) + 1e-8, terms=3)
    assert steps["one_small_term"] == dict(rad=(((1.0 + 1e-7) + 0.5) + 1e-9) + 0.25, terms=5)


def test_steps_headers_are_host_only():
    """No HIP header in the shared steps and the parameter blocks, and one definition of each step: the kernel units call them."""
    import re
    for f in ("ansfm_ms_chain_steps.h", "ansfm_ms_params.h"):
        assert not re.search(r'#\s*include\s*[<"]hip/', open(os.path.join(CSRC, f)).read()), f
    units = "".join(open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.startswith("ansfm_ms_") and f.endswith(".hip.h"))
    assert "conv < 1e-5" not in units                      # the break of the Fourier sum lives in ms_fourier_step alone
    for step in ("ms_surface_element", "ms_doubling_start", "ms_phase_mix", "ms_fourier_step"):
        assert step + "(" in units, step
