"""The index of the k-table's g-fastest copy and the pair clamp of its reads, restated in plain Python (DESIGN.md 3 and 4.1;
gfast_stride, lane_row and load_gas_rows in csrc/ansfm_merge_common.hip.h, k_table_gfast in csrc/ansfm_table_kernels.hip.h).
lnKg[NP][NT][S][Wpad][Gs] with Gs = G rounded up to even; a lane reads the ordinates of one (corner, gas, wavenumber) in batches
of kLoadBatch as 16-byte pairs, a pair that starts past the end clamped to the last pair.  Checked for G = 1 .. 32: every
(corner, gas, wavenumber, ordinate) is consumed exactly once, from the element that holds it; every pair starts 16-byte
aligned; nothing is read outside the copy."""
import os
import re

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "archnemesis_dist_amd", "csrc",
                      "ansfm_merge_common.hip.h")
NP, NT, S, WPAD = 3, 2, 3, 128
CORNERS = ((0, 0), (0, 1), (2, 0), (2, 1))            # (ip, it) of four corner blocks


def gfast_stride(G):
    return (G + 1) & ~1


def corner_offset(ip, it, nu, G):
    """lane_row: the lane's run of gas 0 in block (ip, it), an element offset into lnKg"""
    return (ip * NT + it) * (S * gfast_stride(G) * WPAD) + nu * gfast_stride(G)


def gas_base(s, G):
    """load_gas_rows: the gas advances by Wpad * Gs"""
    return s * WPAD * gfast_stride(G)


def pair_reads(G, batch):
    """load_gas_rows: (first ordinate the pair stands for, element of the run the pair is read from), batch by batch"""
    Gs = gfast_stride(G)
    for g0 in range(0, G, batch):
        for k in range(0, batch, 2):
            yield g0 + k, (g0 + k if g0 + k < Gs else Gs - 2)


def consumed(G, batch):
    """(ordinate, element of the run) for every value that reaches interp_k: r[k] with g0 + k < G"""
    for g, gi in pair_reads(G, batch):
        for half in (0, 1):
            if g + half < G:
                yield g + half, gi + half


def _source_constants():
    text = open(HEADER).read()
    batch = int(re.search(r"constexpr int kLoadBatch = (\d+);", text).group(1))
    stride = re.search(r"constexpr int gfast_stride\(int G\) \{ return ([^;]+); \}", text).group(1)
    return batch, stride


def test_the_source_holds_the_modelled_constants():
    batch, stride = _source_constants()
    assert batch % 2 == 0 and batch == 10
    assert stride.replace(" ", "") == "(G+1)&~1"
    text = open(HEADER).read()
    assert "(g0 + k < Gs) ? g0 + k : Gs - 2" in text                 # the pair clamp
    assert "(size_t)lr.nu * gfast_stride(p.G)" in text                # a wavenumber's run starts at nu * Gs
    assert "p.lnKg + (size_t)s * p.Wpad * Gs" in text                 # the gas advances by Wpad * Gs


@pytest.mark.parametrize("G", range(1, 33))
def test_every_ordinate_is_read_once_from_its_element(G):
    batch, _ = _source_constants()
    Gs = gfast_stride(G)
    index = np.arange(NP * NT * S * WPAD * Gs).reshape(NP, NT, S, WPAD, Gs)      # lnKg's own index
    got = list(consumed(G, batch))
    assert sorted(g for g, _ in got) == list(range(G))                # once each, per (corner, gas, wavenumber)
    assert all(g == e for g, e in got)                                # ordinate g comes from element g of the run
    assert [g for g, _ in got] == list(range(G))                      # ... and in the order the merge stores them
    for ip, it in CORNERS:
        for s in range(S):
            for nu in (0, 1, 63, 64, 69, 70, WPAD - 1):               # real and pad wavenumbers of both blocks
                base = gas_base(s, G) + corner_offset(ip, it, nu, G)
                assert [base + e for _, e in got] == list(index[ip, it, s, nu, :G])


@pytest.mark.parametrize("G", range(1, 33))
def test_pairs_are_aligned_and_inside_the_copy(G):
    batch, _ = _source_constants()
    Gs = gfast_stride(G)
    total = NP * NT * S * WPAD * Gs
    assert Gs % 2 == 0 and G <= Gs <= G + 1
    lo, hi = total, -1
    for ip in range(NP):
        for it in range(NT):
            for s in range(S):
                for nu in range(WPAD):
                    base = gas_base(s, G) + corner_offset(ip, it, nu, G)
                    assert (base * 8) % 16 == 0
                    for _, gi in pair_reads(G, batch):
                        assert gi % 2 == 0 and 0 <= gi <= Gs - 2        # 16-byte aligned, both halves inside the run
                        lo, hi = min(lo, base + gi), max(hi, base + gi + 1)
    assert lo == 0 and hi == total - 1


def test_transposition_fills_every_element():
    """k_table_gfast: block (q, 64 wavenumbers) writes elements (q * Wpad + w0) * Gs + i, i < 64 * Gs, from lnK[(q * G + g) *
    Wpad + w] with w = w0 + i / Gs, g = i % Gs, the pad ordinate boxed 0"""
    for G in (2, 7, 20, 31, 32):
        Gs, Q = gfast_stride(G), NP * NT * S
        lnK = np.arange(Q * G * WPAD, dtype=np.float64).reshape(Q, G, WPAD)
        out = np.full(Q * WPAD * Gs, np.nan)
        written = np.zeros(out.size, int)
        for q in range(Q):
            for w0 in range(0, WPAD, 64):
                for i in range(64 * Gs):
                    w, g = w0 + i // Gs, i % Gs
                    out[(q * WPAD + w0) * Gs + i] = lnK[q, g, w] if g < G else -1.0
                    written[(q * WPAD + w0) * Gs + i] += 1
        assert (written == 1).all()
        out = out.reshape(Q, WPAD, Gs)
        assert np.array_equal(out[:, :, :G], np.transpose(lnK, (0, 2, 1)))
        assert (out[:, :, G:] == -1.0).all()
