"""The layer-grouped lanes of the forward merge at group width 1 (lane_row, lane_tile_of and
TileQueue::next_rows in csrc/ansfm_merge_common.hip.h take the width as run-time data): a tile is 64 consecutive rows of one
wavenumber, running on into the next wavenumber at the end of the row axis.  The plain-Python model of
tests/test_merge_layer_groups_model.py is general in the width; its three properties are run here at nv = 1 over the same
sweeps -- the queue order is a permutation of the block, cell <-> (block, tile, lane) is a bijection onto the Wpad x R cells
whose pad cells are exactly the wavenumbers >= W, and the tiles of one 16-wavenumber span and one row slot are consecutive in
the queue, at most 16 of them -- and the model is tied to the source: the header holds lane_tile_of and lane_cell to two
tables of values by static_assert, and those values are compared with the model here.  Last, at (W, L) = (2, 32) tile 0
holds the same 64 cells at width 1 as at width 2: the exact walk counts of tests/test_merge_rowmajor.py, which are taken on
that one tile, hold for either width."""
import re
from pathlib import Path

import numpy as np
import pytest

from test_merge_layer_groups_model import L_SWEEP, N_SWEEP, W_SWEEP, WAVE, cell_to_tile, lane_cells, queues, tile_of

NV = 1
R_SWEEP = sorted({n * L for n in N_SWEEP for L in L_SWEEP})


def _spots(name):
    """the rows of the constexpr table `name` of the header, which its static_assert holds lane_tile_of / lane_cell to"""
    src = (Path(__file__).resolve().parents[1] / "archnemesis_dist_amd" / "csrc" / "ansfm_merge_common.hip.h").read_text()
    body = re.search(r"constexpr unsigned %s\[\]\[\d\] = \{(.*?)\};" % name, src, re.S).group(1)
    return [tuple(int(v) for v in row.split(",")) for row in re.findall(r"\{([^{}]*)\}", body)]


def test_the_source_gives_the_models_values():
    """The header asserts at compile time that lane_tile_of and lane_cell, the functions the kernel calls, give the values of
    kLaneTileSpots and kLaneCellSpots (and, over sweeps of R, a permutation and a bijection); here the same values are the
    model's: the first, the last and middle tiles of R = 3, 33, 100 and 696 rows and lanes on both sides of a wavenumber seam,
    at both widths."""
    assert "static_assert(lane_spots_hold()" in (Path(__file__).resolve().parents[1] / "archnemesis_dist_amd" / "csrc" /
                                                  "ansfm_merge_common.hip.h").read_text()
    tiles, cells = _spots("kLaneTileSpots"), _spots("kLaneCellSpots")
    assert len(tiles) >= 20 and len(cells) >= 12
    assert {t[2] for t in tiles} == {1, 2} and {t[3] for t in cells} == {1, 2}
    for u, R, nv, k in tiles:
        assert tile_of(u, R, nv) == k, (u, R, nv)
    for k, lane, R, nv, w, row in cells:
        nu, rows = lane_cells(0, k, R, nv)
        assert (int(nu[lane]), int(rows[lane])) == (w, row), (k, lane, R, nv)


@pytest.mark.parametrize("R", R_SWEEP)
def test_queue_order_is_a_permutation_of_the_block(R):
    ks = [tile_of(u, R, NV) for u in range(R)]
    assert sorted(ks) == list(range(R))


@pytest.mark.parametrize("n", N_SWEEP)
@pytest.mark.parametrize("L", L_SWEEP)
@pytest.mark.parametrize("W", W_SWEEP)
def test_cells_and_lanes_are_a_bijection(W, L, n):
    R = n * L
    Wpad = (W + WAVE - 1) // WAVE * WAVE
    tiles = np.array([t for queue in queues(Wpad, R, NV) for t in queue], dtype=np.int64)      # (tiles, 2): block, tile
    vt, k = tiles[:, 0], tiles[:, 1]
    assert vt.min() >= 0 and vt.max() < Wpad // WAVE and k.min() >= 0 and k.max() < R
    nu, row = lane_cells(vt, k, R, NV)                                                        # (tiles, 64)
    assert nu.min() >= 0 and nu.max() < Wpad and row.min() >= 0 and row.max() < R
    assert tiles.shape[0] * WAVE == Wpad * R       # a block is exactly R tiles: nothing is padded along the row axis
    seen = np.bincount((nu * R + row).ravel(), minlength=Wpad * R)
    assert np.all(seen == 1)                       # every cell once: W x R real cells and (Wpad - W) x R pad cells
    pad = nu >= W                                  # the pad cells are exactly the wavenumbers >= W, every row of them
    assert int(pad.sum()) == (Wpad - W) * R
    assert np.array_equal(np.sort((nu * R + row)[pad]), np.arange(W * R, Wpad * R))
    # a tile is rows of one wavenumber, or the end of one wavenumber's rows and the start of the next ones'
    assert np.all(np.diff(nu, axis=1) >= 0) and np.all(np.diff(nu, axis=1) <= 1)
    same = np.diff(nu, axis=1) == 0
    assert np.all(np.diff(row, axis=1)[same] == 1) and np.all(row[:, 1:][~same] == 0)
    # and back, lane by lane
    bvt, bk, blane = cell_to_tile(nu, row, R, NV)
    assert np.array_equal(bvt, np.broadcast_to(vt[:, None], nu.shape)) and np.array_equal(bk, np.broadcast_to(k[:, None], nu.shape))
    assert np.array_equal(blane, np.broadcast_to(np.arange(WAVE), nu.shape))


@pytest.mark.parametrize("R", R_SWEEP)
def test_tiles_of_one_span_and_row_slot_are_neighbours(R):
    """A tile's slot = how many tiles start before it in its wavenumber.  The tiles of one slot that start in the 16
    wavenumbers of one span read the same 128-byte table lines: they are consecutive in the queue, at most 16 of them, their
    first rows lie within one tile's rows of each other, and the slots go out in ascending order."""
    Q = WAVE // NV
    order = [tile_of(u, R, NV) for u in range(R)]
    grp = [k * Q // R for k in order]
    slot = [k - (g * R + Q - 1) // Q for k, g in zip(order, grp)]
    row0 = [k * Q - g * R for k, g in zip(order, grp)]
    assert min(slot) >= 0 and slot == sorted(slot)
    classes = {}
    for u, (g, s) in enumerate(zip(grp, slot)):
        classes.setdefault((s, g * NV // 16), []).append(u)
    for (s, span), us in classes.items():
        assert us == list(range(us[0], us[0] + len(us))), (s, span, us)
        assert len(us) <= 16 // NV
        assert max(row0[u] for u in us) - min(row0[u] for u in us) < Q
        assert [grp[u] for u in us] == sorted(grp[u] for u in us)


def test_tiles_of_a_block_stay_in_one_queue():
    for qi, queue in enumerate(queues(576, 33, NV)):
        assert all(vt % 8 == qi for vt, _ in queue)
        blocks = [vt for vt, _ in queue]
        assert blocks == sorted(blocks)            # a block's tiles are handed out together


def test_the_one_tile_of_the_exact_counts_is_the_same_at_both_widths():
    """(W, L) = (2, 32): 2 wavenumbers x 32 rows.  Tile 0 of block 0 holds these 64 cells at width 2 (one tile) and at width 1
    (32 rows of wavenumber 0, running on into the 32 rows of wavenumber 1); it is the first tile either queue hands out, and
    every other tile of the block holds pad cells only."""
    W, L = 2, 32
    cells = {(w, r) for w in range(W) for r in range(L)}
    for nv in (1, 2):
        assert tile_of(0, L, nv) == 0
        nu, row = lane_cells(0, 0, L, nv)
        assert set(zip(nu.tolist(), row.tolist())) == cells
        for k in range(1, L):
            assert lane_cells(0, k, L, nv)[0].min() >= W
