"""A model in plain Python of the forward merge's layer-grouped lanes (LaneRow, lane_tile_of and
TileQueue::next_rows in csrc/ansfm_merge_common.hip.h): the cells of a 64-wavenumber block numbered (wavenumber / NV, row,
wavenumber % NV), a tile = 64 consecutive cells, the R = n_models * L tiles of a block handed out slot by slot.  Checked here:
cell -> (queue, position, lane) and back is a bijection onto the Wpad x R cells, the pad cells are the wavenumbers >= W, a row
splits into (model, layer) as the kernel's amount index needs, and the queue order keeps the tiles that share a
16-wavenumber span and a row slot next to each other."""
import re
from pathlib import Path

import numpy as np
import pytest

WAVE = 64
NVS = (2, 4, 8)
W_SWEEP = (1, 63, 64, 70, 136, 576)
L_SWEEP = (1, 3, 7, 31, 32, 33, 100)
N_SWEEP = (1, 3)


def tile_of(u, R, nv):
    """lane_tile_of: the u-th tile a block hands out, as its index in the block's cell order"""
    Q = WAVE // nv
    fl, rem = divmod(R, Q)
    if u < Q * fl:
        slot, grp = divmod(u, Q)
    else:
        slot, grp = fl, (u - Q * fl) * Q // rem
    return (grp * R + Q - 1) // Q + slot


def lane_cells(vt, k, R, nv):
    """lane_row: (wavenumber, row) of the 64 lanes of tile k of block vt; vt, k scalars or arrays of tiles (one row each)"""
    c = np.asarray(k)[..., None] * WAVE + np.arange(WAVE)
    pair = c // nv
    grp = pair // R
    return np.asarray(vt)[..., None] * WAVE + grp * nv + c % nv, pair - grp * R


def cell_to_tile(nu, row, R, nv):
    """the inverse: (block, tile of the block's cell order, lane) of a cell"""
    vt, w = divmod(nu, WAVE)
    c = ((w // nv) * R + row) * nv + w % nv
    return vt, c // WAVE, c % WAVE


def queues(Wpad, R, nv):
    """TileQueue::next_rows: for each of the eight queues the (block, tile) pairs in the order the counter hands them out"""
    nvt = Wpad // WAVE
    out = []
    for q in range(8):
        nvt_q = (nvt - q + 7) // 8
        out.append([(q + 8 * (t // R), tile_of(t % R, R, nv)) for t in range(nvt_q * R)])
    return out


def test_group_width_in_the_source_is_one_of_the_modelled():
    src = (Path(__file__).resolve().parents[1] / "archnemesis_dist_amd" / "csrc" / "ansfm_merge_plan.h").read_text()
    nv = int(re.search(r"constexpr int kLaneNV = (\d+);", src).group(1))
    assert nv in NVS


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("R", sorted({n * L for n in N_SWEEP for L in L_SWEEP}))
def test_queue_order_is_a_permutation_of_the_block(R, nv):
    ks = [tile_of(u, R, nv) for u in range(R)]
    assert sorted(ks) == list(range(R))


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("n", N_SWEEP)
@pytest.mark.parametrize("L", L_SWEEP)
@pytest.mark.parametrize("W", W_SWEEP)
def test_cells_and_lanes_are_a_bijection(W, L, n, nv):
    R = n * L
    Wpad = (W + WAVE - 1) // WAVE * WAVE
    tiles = np.array([t for queue in queues(Wpad, R, nv) for t in queue], dtype=np.int64)      # (tiles, 2): block, tile
    vt, k = tiles[:, 0], tiles[:, 1]
    assert vt.min() >= 0 and vt.max() < Wpad // WAVE and k.min() >= 0 and k.max() < R
    nu, row = lane_cells(vt, k, R, nv)                                                        # (tiles, 64)
    assert nu.min() >= 0 and nu.max() < Wpad and row.min() >= 0 and row.max() < R
    assert tiles.shape[0] * WAVE == Wpad * R       # nothing is padded along the row axis
    seen = np.bincount((nu * R + row).ravel(), minlength=Wpad * R)
    assert np.all(seen == 1)                       # every cell once: W x R real cells and (Wpad - W) x R pad cells
    # and back, lane by lane
    bvt, bk, blane = cell_to_tile(nu, row, R, nv)
    assert np.array_equal(bvt, np.broadcast_to(vt[:, None], nu.shape)) and np.array_equal(bk, np.broadcast_to(k[:, None], nu.shape))
    assert np.array_equal(blane, np.broadcast_to(np.arange(WAVE), nu.shape))
    # a row is (model, layer); gas s of that row reads amount[n][S][L] at (m * S) * L + l + s * L
    S = 5
    rows = np.arange(R)
    m, l = rows // L, rows % L
    amount_index = np.arange(n * S * L).reshape(n, S, L)
    for s in (0, S - 1):
        assert np.array_equal(m * S * L + l + s * L, amount_index[m, s, l])


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("R", sorted({n * L for n in N_SWEEP for L in L_SWEEP}))
def test_tiles_of_one_span_and_row_slot_are_neighbours(R, nv):
    """A tile's slot = how many tiles start before it in its wavenumber group.  The tiles of one slot that start in the
    16 / NV groups of one 16-wavenumber span read the same 128-byte table lines: they are consecutive in the queue, their first
    rows lie within one tile's rows of each other, and the slots go out in ascending order."""
    Q = WAVE // nv
    order = [tile_of(u, R, nv) for u in range(R)]
    grp = [k * Q // R for k in order]
    slot = [k - (g * R + Q - 1) // Q for k, g in zip(order, grp)]
    row0 = [k * Q - g * R for k, g in zip(order, grp)]
    assert min(slot) >= 0 and slot == sorted(slot)
    classes = {}
    for u, (g, s) in enumerate(zip(grp, slot)):
        classes.setdefault((s, g * nv // 16), []).append(u)
    for (s, span), us in classes.items():
        assert us == list(range(us[0], us[0] + len(us))), (s, span, us)
        assert len(us) <= 16 // nv
        assert max(row0[u] for u in us) - min(row0[u] for u in us) < Q
        assert [grp[u] for u in us] == sorted(grp[u] for u in us)


def test_tiles_of_a_block_stay_in_one_queue():
    for nv in NVS:
        for qi, queue in enumerate(queues(576, 33, nv)):
            assert all(vt % 8 == qi for vt, _ in queue)
            blocks = [vt for vt, _ in queue]
            assert blocks == sorted(blocks)            # a block's tiles are handed out together
