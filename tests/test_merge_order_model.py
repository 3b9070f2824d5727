"""The wavenumber order of the forward merge at group width 1 (merge_order_key, merge_order_rank and
merge_order_inverse in csrc/ansfm_merge_common.hip.h): the 64 wavenumbers of a block are handed out sorted by the pattern byte
the launch before wrote for them, pad wavenumbers (byte 0xFF) behind the real ones, equal bytes in wavenumber order.  A plain-
Python model of rank / inverse / cell mapping: whatever the bytes are, the cells of a block's R tiles are a bijection onto its
64 x R cells and the pad cells are exactly the wavenumbers >= W; all-zero bytes give the mapping of
tests/test_merge_one_wavenumber_model.py.  The model is tied to the source by the header's static_assert over kOrderSpots,
whose values are compared with the model here."""
import re
from pathlib import Path

import numpy as np
import pytest

from test_merge_one_wavenumber_model import NV, lane_cells

WAVE = 64
R_SWEEP = (1, 3, 33, 64, 65, 100, 696)
HEADER = Path(__file__).resolve().parents[1] / "archnemesis_dist_amd" / "csrc" / "ansfm_merge_common.hip.h"


def order_rank(block_bytes):
    """merge_order_rank for the 64 wavenumbers of a block: the number of smaller keys (byte << 6) | wavenumber"""
    key = (np.asarray(block_bytes, dtype=np.int64) << 6) | np.arange(WAVE)
    return np.array([int(np.sum(key < k)) for k in key])


def order_inverse(block_bytes):
    """merge_order_inverse: the wavenumber at each position (lane i sends i to lane rank(i))"""
    rank = order_rank(block_bytes)
    assert sorted(rank.tolist()) == list(range(WAVE))
    inv = np.empty(WAVE, dtype=np.int64)
    inv[rank] = np.arange(WAVE)
    return inv


def block_bytes(hint, vt, W):
    """what the wave reads for block vt: the launch before's byte of a real wavenumber, 0xFF for a pad wavenumber"""
    nu = vt * WAVE + np.arange(WAVE)
    return np.where(nu < W, np.asarray(hint)[np.minimum(nu, len(hint) - 1)], 0xFF)


def ordered_lane_cells(vt, k, R, hint, W):
    """lane_row with the order: (wavenumber, row) of the 64 lanes of tile k of block vt"""
    pos, row = lane_cells(0, k, R, NV)             # the cell order's wavenumber index is a position in the block's order
    return vt * WAVE + order_inverse(block_bytes(hint, vt, W))[pos], row


def hints(kind, Wpad, rng):
    if kind == "random":
        return rng.integers(0, 256, Wpad)
    if kind == "few patterns":
        return rng.choice([0x00, 0x80, 0xC0, 0xFE, 0xFF], Wpad)
    if kind == "all equal":
        return np.full(Wpad, 0xA0)
    if kind == "all distinct":                     # within a block: a permutation of 64 values, the top bits varying
        return np.concatenate([rng.permutation(WAVE) * 4 for _ in range(Wpad // WAVE)])
    if kind == "descending":
        return np.tile(np.arange(WAVE)[::-1] * 4, Wpad // WAVE)
    assert kind == "zero"
    return np.zeros(Wpad, dtype=np.int64)


KINDS = ("random", "few patterns", "all equal", "all distinct", "descending", "zero")


def _spots():
    src = HEADER.read_text()
    body = re.search(r"constexpr unsigned kOrderSpots\[\]\[2\] = \{(.*?)\};", src, re.S).group(1)
    consts = {n: int(v, 0) for n, v in re.findall(r"\b(kOrderSpot\w+) = (\w+)", src)}
    return [tuple(int(v) for v in row.split(",")) for row in re.findall(r"\{([^{}]*)\}", body)], consts


def test_the_source_gives_the_models_values():
    """The header asserts at compile time that merge_order_rank, over the keys the kernel forms, gives the positions of
    kOrderSpots for the bytes of merge_order_spot_byte (58 real wavenumbers of eight patterns, six pads), and the identity for
    all-zero bytes; here the same positions are the model's."""
    src = HEADER.read_text()
    assert 'static_assert(order_spots_hold()' in src
    assert "return (byte << 6) | i;" in src        # merge_order_key
    spots, c = _spots()
    assert len(spots) >= 10
    i = np.arange(WAVE)
    b = np.where(i < c["kOrderSpotReal"], (i * c["kOrderSpotMul"] + c["kOrderSpotAdd"]) & c["kOrderSpotMask"], 0xFF)
    assert len(set(b[:c["kOrderSpotReal"]].tolist())) >= 6
    rank = order_rank(b)
    for w, pos in spots:
        assert rank[w] == pos, (w, pos, rank[w])
    assert {w for w, _ in spots} & set(range(c["kOrderSpotReal"], WAVE))      # a pad wavenumber among them
    assert any(w != pos for w, pos in spots)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R", R_SWEEP)
@pytest.mark.parametrize("W", [64, 70, 1])
def test_cells_of_a_block_are_a_bijection(W, R, kind):
    """every cell of the Wpad x R cells once, whatever the bytes; the pad cells are exactly the wavenumbers >= W, and they are
    the last positions of their block, so that the tiles that hold nothing but pad cells are those of the identity order"""
    rng = np.random.default_rng(1000 * W + R)
    Wpad = (W + WAVE - 1) // WAVE * WAVE
    hint = hints(kind, Wpad, rng)
    for vt in range(Wpad // WAVE):
        nu, row = zip(*(ordered_lane_cells(vt, k, R, hint, W) for k in range(R)))
        nu, row = np.array(nu), np.array(row)
        assert nu.min() >= vt * WAVE and nu.max() < (vt + 1) * WAVE and row.min() >= 0 and row.max() < R
        seen = np.bincount(((nu - vt * WAVE) * R + row).ravel(), minlength=WAVE * R)
        assert np.all(seen == 1)
        ident_nu, ident_row = lane_cells(vt, np.arange(R), R, NV)
        assert np.array_equal(row, ident_row)      # the order moves wavenumbers, never rows
        assert np.array_equal(nu >= W, ident_nu >= W)
        assert int((nu >= W).sum()) == max(0, (vt + 1) * WAVE - max(W, vt * WAVE)) * R
        # a tile is still rows of one wavenumber, or the end of one wavenumber's rows and the start of the next one's in the order
        for k in range(R):
            changes = np.flatnonzero(np.diff(nu[k]) != 0)
            assert np.all(row[k][changes + 1] == 0) and np.all(row[k][changes] == R - 1)


@pytest.mark.parametrize("R", R_SWEEP)
def test_zero_bytes_give_the_committed_mapping(R):
    W = 70
    hint = hints("zero", 128, None)
    for vt in range(2):
        for k in range(R):
            nu, row = ordered_lane_cells(vt, k, R, hint, W)
            ref_nu, ref_row = lane_cells(vt, k, R, NV)
            assert np.array_equal(nu, ref_nu) and np.array_equal(row, ref_row)


def test_equal_bytes_keep_wavenumber_order_and_pads_stay_behind():
    assert np.array_equal(order_inverse(np.full(WAVE, 0xA0)), np.arange(WAVE))
    # real wavenumbers whose byte is 0xFF (eight merges, all row-major) tie with the pads and stay in front of them
    b = block_bytes(np.full(128, 0xFF), 1, 70)
    assert np.array_equal(order_inverse(b), np.arange(WAVE))
    # two patterns: the wavenumbers of the smaller byte first, each group in wavenumber order
    b = np.where(np.arange(WAVE) % 2 == 0, 0x80, 0x00)
    assert np.array_equal(order_inverse(b), np.concatenate([np.arange(1, WAVE, 2), np.arange(0, WAVE, 2)]))
