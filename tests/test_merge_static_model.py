"""The static schedule of a whole row-major walk (merge_static_build in csrc/ansfm_merge_plan.h) against a
plain-Python model, no GPU: the recurrence of merge_walk_nodiv on wave-uniform data -- w = float32(del_g[i]) * float32(del_g[j])
as a float32 product widened, gdn = gd + w, a crossing where gdn >= g_ord[ig + 1] (ordered, NaN behind the last bin), one bin per
element -- in NumPy float32 / float64.  The host builder is printed by tests/host/merge_static_main.cpp, built with the host
compiler and its sanitizers and run as a child process; every double is compared by its bits.

The model also replays one lane: merge_walk_nodiv element by element over a row-major merge, and the static form (cv and one
fma per element, fma(C1, cv, kacc) and C2 * cv at the builder's crossings) on the same operands.  Every closed bin and the end
state must agree bit for bit.  fma is the exact one (rational arithmetic, rounded once)."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "archnemesis_dist_amd", "csrc")
FLT_MIN = float(np.finfo(np.float32).tiny)


def gauss_legendre_f32(G):
    from archnemesis_dist_amd import synthetic as syn
    return syn.gauss_legendre_01(G, as_float32=True)[1].astype(np.float32).astype(np.float64)


def interior_delg(G=20):
    """Crossings at interior columns, four in one row: three tiny bins between two large ones, and weights that sum to 0.98, so
    that the walk lags behind the boundaries and passes the three tiny bins inside the large weight's row (columns 0 .. 3 of
    row 4).  The last weight is large enough for the walk to end inside the last bin."""
    d = np.full(G, (0.98 - 0.7003 - 0.1) / (G - 6))
    d[:5] = [0.2, 1e-4, 1e-4, 1e-4, 0.5]
    d[G - 1] = 0.1
    return d.astype(np.float32).astype(np.float64)


def invalid_delg(G=20):
    """Weights that sum to 1.02: the walk runs ahead of the boundaries, and by the top rows, whose weights are smaller than its
    lead, it closes bin b before row b -- no on-chip placement"""
    return (1.02 * gauss_legendre_f32(G)).astype(np.float32).astype(np.float64)


def g_ord_f32(delg):
    G = len(delg)
    acc = np.float32(0.0)
    g = np.zeros(G + 2)
    with np.errstate(all="ignore"):
        for k in range(G):
            acc = np.float32(acc + np.float32(delg[k]))
            g[k + 1] = float(acc)
    g[G] = 1.0
    g[G + 1] = np.nan
    return g


def weights_f32(delg):
    f = np.asarray(delg, np.float64).astype(np.float32)
    with np.errstate(all="ignore"):
        return np.multiply.outer(f, f).astype(np.float32), f


def schedule_model(delg):
    """dict(valid, nbins, gd_end, last_width, masks, c1, c2) by the walk's recurrence"""
    G = len(delg)
    g = g_ord_f32(delg)
    wf, f = weights_f32(delg)

    def plain(v):
        v = abs(float(v))
        return v == 0.0 or (FLT_MIN <= v < np.inf)
    ok = all(plain(v) for v in f) and all(plain(v) for v in wf.ravel())
    gd, ig = 0.0, 0
    masks, c1, c2 = [0] * G, [], []
    for i in range(G):
        for j in range(G):
            gdn = gd + float(wf[i, j])
            if ig < G and gdn >= g[ig + 1]:
                ok = ok and ig <= i
                masks[i] |= 1 << j
                c1.append(g[ig + 1] - gd)
                c2.append(gdn - g[ig + 1])
                ig += 1
            gd = gdn
    return dict(valid=int(ok), nbins=ig, gd_end=gd, last_width=gd - g[G - 1], masks=masks, c1=c1, c2=c2)


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def replay_walk(delg, rows, cols):
    """merge_walk_nodiv over the row-major order for one lane: (closed sums, kacc, gd, bins)"""
    G = len(delg)
    g = g_ord_f32(delg)
    wf, _ = weights_f32(delg)
    gd, kacc, ig, gnext, closed = 0.0, 0.0, 0, g[1], []
    for i in range(G):
        for j in range(G):
            cv, w = rows[i] + cols[j], float(wf[i, j])
            gdn = gd + w
            kn = fma(cv, w, kacc)
            if gdn >= gnext:
                closed.append(fma(gnext - gd, cv, kacc))
                kn = (gdn - gnext) * cv
                ig += 1
                gnext = g[ig + 1]
            kacc, gd = kn, gdn
    return closed, kacc, gd, ig


def replay_static(delg, sched, rows, cols):
    """the static form on the builder's schedule: no gd, no compare"""
    G = len(delg)
    wf, _ = weights_f32(delg)
    kacc, n, closed = 0.0, 0, []
    for i in range(G):
        for j in range(G):
            cv = rows[i] + cols[j]
            if (sched["masks"][i] >> j) & 1:
                closed.append(fma(sched["c1"][n], cv, kacc))
                kacc = sched["c2"][n] * cv
                n += 1
            else:
                kacc = fma(cv, float(wf[i, j]), kacc)
    return closed, kacc, sched["gd_end"], n


CASES = [(f"gl{G}", gauss_legendre_f32(G)) for G in (2, 3, 8, 10, 12, 16, 17, 20, 32)] + [
    ("interior", interior_delg()),
    ("open_last", np.array([0.25, 0.25, 0.25, 0.2])),
    ("closes_on_last", np.full(16, 1.0 / 16)),
    ("invalid", invalid_delg()),
    ("invalid4", np.full(4, 0.5)),
    ("nan", np.array([0.1, 0.2, np.nan, 0.3, 0.4])),
    ("nan_first", np.array([np.nan, 0.5, 0.5])),
]


def _compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


def _bits(v):
    return np.float64(v).view(np.uint64)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("merge_static") / "merge_static_main")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all"] + static + ["-I", CSRC, os.path.join(ROOT, "tests", "host", "merge_static_main.cpp"), "-o", exe],
                   check=True, timeout=300)
    text = "".join(name + " " + " ".join(float(v).hex() for v in d) + "\n" for name, d in CASES)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        name, *fields = line.split()
        kv = dict(f.split("=") for f in fields)
        lst = lambda s, conv: [conv(x) for x in s.split(",")] if s else []
        out[name] = dict(valid=int(kv["valid"]), nbins=int(kv["nbins"]), gd_end=float.fromhex(kv["gd_end"]),
                         last_width=float.fromhex(kv["last_width"]), masks=lst(kv["masks"], int),
                         c1=lst(kv["c1"], float.fromhex), c2=lst(kv["c2"], float.fromhex))
    assert set(out) == {name for name, _ in CASES}
    return out


@pytest.mark.parametrize("name,delg", CASES, ids=[c[0] for c in CASES])
def test_builder_is_the_model(built, name, delg):
    host, model = built[name], schedule_model(delg)
    assert host["valid"] == model["valid"] and host["nbins"] == model["nbins"] and host["masks"] == model["masks"], (host, model)
    for key in ("gd_end", "last_width"):
        assert _bits(host[key]) == _bits(model[key]), key
    for key in ("c1", "c2"):
        assert len(host[key]) == host["nbins"] == len(model[key])
        assert all(_bits(a) == _bits(b) for a, b in zip(host[key], model[key])), key
    assert sum(bin(m).count("1") for m in host["masks"]) == host["nbins"] <= len(delg)
    assert all(m < (1 << len(delg)) for m in host["masks"])


def test_what_the_cases_are_for(built):
    """each constructed del_g does what it was constructed for"""
    G = 20
    inner = built["interior"]
    assert inner["valid"] == 1 and inner["nbins"] == G - 1 and max(bin(m).count("1") for m in inner["masks"]) >= 3
    assert any(m & ~(1 | 1 << (G - 1)) for m in inner["masks"]), "a crossing at an interior column"
    assert built["open_last"]["valid"] == 1 and built["open_last"]["nbins"] < 4
    last = built["closes_on_last"]
    assert last["valid"] == 1 and last["nbins"] == 16 and last["masks"][15] >> 15 == 1
    assert built["invalid"]["valid"] == 0 and built["invalid4"]["valid"] == 0
    # NaN: invalid, nothing crosses from the first NaN weight on, and the masks name existing columns only
    for name in ("nan", "nan_first"):
        assert built[name]["valid"] == 0 and np.isnan(built[name]["gd_end"])
    assert built["nan_first"]["nbins"] == 0 and built["nan"]["nbins"] == 0
    # the Gauss-Legendre schedules: valid, at most two crossings per row, at the row's first or last column
    for Gl in (8, 10, 12, 16, 17, 20, 32):
        s = built[f"gl{Gl}"]
        assert s["valid"] == 1 and Gl - 1 <= s["nbins"] <= Gl
        assert all(m & ~(1 | 1 << (Gl - 1)) == 0 for m in s["masks"]), s["masks"]


@pytest.mark.parametrize("name,delg", [c for c in CASES if not c[0].startswith("nan")], ids=[c[0] for c in CASES if not c[0].startswith("nan")])
def test_static_form_is_the_walk(built, name, delg):
    """one lane, either way round: the closed sums, the open bin's kacc, gd and the bin count, bit for bit -- with the builder's
    schedule, valid or not (validity is about where the closed sums can be kept, not about their values)"""
    G = len(delg)
    rng = np.random.default_rng(G)
    big = np.sort(rng.uniform(1.0, 50.0, G)) * 1e-3
    small = np.sort(rng.uniform(1.0, 50.0, G)) * 1e-9
    for rows, cols in ((big, small), (small, big)):
        want = replay_walk(delg, rows, cols)
        got = replay_static(delg, built[name], rows, cols)
        assert len(want[0]) == len(got[0]) == want[3] == got[3]
        assert all(_bits(a) == _bits(b) for a, b in zip(want[0], got[0]))
        assert _bits(want[1]) == _bits(got[1]) and _bits(want[2]) == _bits(got[2])
