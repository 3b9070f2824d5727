"""CPU-only: the host planning of per-model phase functions in the multiple-scattering batch (csrc/ansfm_ms_variants.h), run by
tests/host/ms_variants_main.cpp, which is built with the host compiler under AddressSanitizer and UBSan and run as a child
process.  The expectations come from NumPy on the same arrays: which (variant, population) pairs differ from variant 0 in any
bit, the launch list, the offsets of a variant's phase matrices and Hansen factors, and the validation of a pending setting."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "archnemesis_dist_amd", "csrc")

# name: sizes, the setting (n_models, ncont, nth as set; phase_of), the call's (n_models, ncont, nth), tags [V][ncont], perturbations
CASES = {
    # the GPU tests' six models: population 0 differs in variant 1, population 1 in variant 2 (one element, far into the block)
    "six_models": dict(V=3, ncont=2, iray=1, W=7, nth=5, nf=2, nmu=5, G=3, set=(6, 2, 5), call=(6, 2, 5), phase_of=[0, 0, 1, 1, 2, 1],
                       tags=[[1, 2], [3, 2], [1, 2]], pert=[(2, 1, 7 * 2 * 5 - 1, 2.5)]),
    # no component differs at all: the variants are copies; nothing but variant 0's components is launched
    "copies": dict(V=3, ncont=2, iray=1, W=4, nth=3, nf=1, nmu=16, G=2, set=(3, 2, 3), call=(3, 2, 3), phase_of=[0, 2, 1],
                   tags=[[1, 2], [1, 2], [1, 2]], pert=[]),
    # bits, not values: -0.0 against 0.0 differs; no Rayleigh: variant 0's list has the aerosols only
    "signed_zero": dict(V=2, ncont=3, iray=0, W=3, nth=4, nf=0, nmu=4, G=4, set=(2, 3, 4), call=(2, 3, 4), phase_of=[0, 1],
                        tags=[[0, 0, 0], [0, 0, 0]], pert=[(1, 1, 0, -0.0)]),
    # every population differs in every variant
    "all_differ": dict(V=4, ncont=2, iray=1, W=2, nth=3, nf=3, nmu=8, G=2, set=(5, 2, 3), call=(5, 2, 3), phase_of=[0, 3, 3, 1, 2],
                       tags=[[1, 2], [3, 4], [5, 6], [7, 8]], pert=[]),
    # V = 1: not armed; the plan is variant 0 alone
    "one_variant": dict(V=1, ncont=1, iray=1, W=5, nth=3, nf=2, nmu=6, G=2, set=(2, 1, 3), call=(2, 1, 3), phase_of=[0, 0],
                        tags=[[1]], pert=[]),
    # refusals
    "entry_too_large": dict(V=2, ncont=1, iray=1, W=2, nth=3, nf=0, nmu=4, G=2, set=(3, 1, 3), call=(3, 1, 3), phase_of=[0, 2, 1],
                            tags=[[1], [2]], pert=[]),
    "entry_negative": dict(V=2, ncont=1, iray=1, W=2, nth=3, nf=0, nmu=4, G=2, set=(3, 1, 3), call=(3, 1, 3), phase_of=[0, -1, 1],
                           tags=[[1], [2]], pert=[]),
    "model_0_not_variant_0": dict(V=2, ncont=1, iray=1, W=2, nth=3, nf=0, nmu=4, G=2, set=(3, 1, 3), call=(3, 1, 3), phase_of=[1, 0, 1],
                                  tags=[[1], [2]], pert=[]),
    "other_n_models": dict(V=2, ncont=1, iray=1, W=2, nth=3, nf=0, nmu=4, G=2, set=(3, 1, 3), call=(4, 1, 3), phase_of=[0, 0, 1],
                           tags=[[1], [2]], pert=[]),
    "other_ncont": dict(V=2, ncont=1, iray=1, W=2, nth=3, nf=0, nmu=4, G=2, set=(3, 1, 3), call=(3, 2, 3), phase_of=[0, 0, 1],
                        tags=[[1], [2]], pert=[]),
    "other_nth": dict(V=2, ncont=1, iray=1, W=2, nth=3, nf=0, nmu=4, G=2, set=(3, 1, 3), call=(3, 1, 4), phase_of=[0, 0, 1],
                      tags=[[1], [2]], pert=[]),
}


def _compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ms_variants") / "ms_variants_main")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all"] + static + ["-I", CSRC, os.path.join(ROOT, "tests", "host", "ms_variants_main.cpp"), "-o", exe],
                   check=True, timeout=300)
    lines = []
    for name, c in CASES.items():
        f = [name] + [c[k] for k in ("V", "ncont", "iray", "W", "nth", "nf", "nmu", "G")] + list(c["set"]) + list(c["call"]) + c["phase_of"]
        f += [t for row in c["tags"] for t in row] + [len(c["pert"])]
        for v, pop, idx, val in c["pert"]:
            f += [v, pop, idx, float(val).hex()]
        lines.append(" ".join(str(x) for x in f))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        name, *fields = line.split()
        out[name] = dict(f.split("=", 1) for f in fields)
    assert set(out) == set(CASES)
    return out


def _arrays(c):
    """the variants' phase arrays [V][ncont][W][2][nth] as the program fills them"""
    a = np.empty((c["V"], c["ncont"], c["W"], 2, c["nth"]))
    a[:] = np.asarray(c["tags"], dtype=np.float64)[:, :, None, None, None]
    for v, pop, idx, val in c["pert"]:
        a[v, pop].reshape(-1)[idx] = val
    return a


def _expected(c):
    a = _arrays(c)
    V, ncont, ncomp = c["V"], c["ncont"], c["ncont"] + 1
    diff = np.zeros((V, ncomp), dtype=int)
    for v in range(1, V):
        for pop in range(ncont):
            diff[v, pop] = a[v, pop].tobytes() != a[0, pop].tobytes()
    pairs = [(0, pop) for pop in range(ncont)] + ([(0, ncont)] if c["iray"] > 0 else [])
    npairs0 = len(pairs)
    pairs += [(v, pop) for v in range(1, V) for pop in range(ncont) if diff[v, pop]]
    nn = c["nmu"] ** 2
    nph = c["W"] * (c["nf"] + 1) * ncomp * nn
    nfc = c["G"] * c["W"] * ncomp * nn
    vstride = 2 * nph + nfc
    return dict(npairs0=npairs0, pairs=pairs, diff=diff, nph=nph, nfc=nfc, vstride=vstride, total=V * vstride,
                st_phas=ncont * c["W"] * 2 * c["nth"], bytes=(V - 1) * vstride * 8,
                off=[(v * vstride, v * vstride + nph, v * vstride + 2 * nph) for v in range(V)])


@pytest.mark.parametrize("name", ["six_models", "copies", "signed_zero", "all_differ", "one_variant"])
def test_pairs_layout_and_offsets(planned, name):
    got, want = planned[name], _expected(CASES[name])
    assert got["valid"] == "1" and got["armed"] == ("1" if CASES[name]["V"] > 1 else "0")
    pairs = [tuple(int(x) for x in p.split(":")) for p in got["pairs"].split(",")] if got["pairs"] else []
    assert pairs == want["pairs"] and int(got["npairs"]) == len(pairs) and int(got["npairs0"]) == want["npairs0"]
    assert got["diff"] == "".join(str(d) for d in want["diff"].reshape(-1))
    for k in ("nph", "nfc", "vstride", "total", "st_phas", "bytes"):
        assert int(got[k]) == want[k], k
    assert [tuple(int(x) for x in o.split(":")) for o in got["off"].split(",")] == want["off"]
    assert [int(x) for x in got["ndiff"].split(",")] == list(want["diff"].sum(axis=1))


def test_expected_pairs_of_the_named_cases(planned):
    """the NumPy expectation itself, spelled out where it is short"""
    assert planned["six_models"]["pairs"] == "0:0,0:1,0:2,1:0,2:1"
    assert planned["copies"]["pairs"] == "0:0,0:1,0:2" and planned["copies"]["ndiff"] == "0,0,0"      # no differing component at all
    assert planned["signed_zero"]["pairs"] == "0:0,0:1,0:2,1:1"
    assert planned["one_variant"]["pairs"] == "0:0,0:1"
    # the variants' buffers never overlap and follow variant 0's without a gap
    off = [tuple(int(x) for x in o.split(":")) for o in planned["all_differ"]["off"].split(",")]
    stride = int(planned["all_differ"]["vstride"])
    assert all(off[v + 1][0] == off[v][0] + stride and off[v][0] < off[v][1] < off[v][2] < off[v + 1][0] for v in range(3))


@pytest.mark.parametrize("name", ["entry_too_large", "entry_negative", "model_0_not_variant_0", "other_n_models", "other_ncont",
                                  "other_nth"])
def test_validation_refuses(planned, name):
    assert planned[name]["valid"] == "0" and "pairs" not in planned[name]


def test_planning_header_is_host_only():
    text = open(os.path.join(CSRC, "ansfm_ms_variants.h")).read()
    assert not re.search(r'#\s*include\s*[<"]hip/', text)
    assert "ansfm_ms_variants.h" in open(os.path.join(CSRC, "ansfm_ctx.hip.h")).read()
