"""The 11-bit key packing of the forward merge (csrc/ansfm_merge64.hip.h) restated in plain Python: the next key of a popped
row formed as "winner's low word + 32, inserted under the mask 0x7FF" (pack_key11_next) against the field-by-field packing
(pack_key11) for every (row, column), and the index of the weight product table WT[(col << 5) | row] for every list length
instantiated.  No GPU: this pins the argument, tests/test_merge_weight_table.py pins the kernel."""
import random
import struct

import pytest

MASK = 0x7FF
LIST_LENGTHS = [8, 10, 16, 20, 32]


def bits(v):
    return struct.unpack('<Q', struct.pack('<d', v))[0]


def pack(v, row, col):
    """pack_key11: the value's low 11 mantissa bits replaced by (col << 5) | row."""
    return (bits(v) & ~MASK) | ((col << 5) | row)


def dec(key):
    """merge_fetch: row = bits 0-4, column = bits 5-10 of the key's low word."""
    kb = key & 0xFFFFFFFF
    return kb & 31, (kb >> 5) & 63


def pack_next(v, kw):
    """pack_key11_next: v_add_u32 kw + 32 (wraps at 32 bits), v_bfi_b32 under the mask into the value's low word."""
    b = bits(v)
    lo = (((kw + 32) & 0xFFFFFFFF) & MASK) | ((b & 0xFFFFFFFF) & ~MASK & 0xFFFFFFFF)
    return (b & 0xFFFFFFFF00000000) | lo


def test_low_word_plus_32_under_the_mask_is_row_and_next_column():
    rnd = random.Random(11)
    for row in range(32):
        for col in range(33):                       # col <= 32: column G of a 32-entry merge is the sentinel's
            for _ in range(8):
                vw = rnd.choice([0.0, 1.0, 10 ** rnd.uniform(-30, 30), struct.unpack('<d', struct.pack('<Q', rnd.getrandbits(63)))[0]])
                if vw != vw:
                    continue
                vn = rnd.choice([0.0, 10 ** rnd.uniform(-30, 30), struct.unpack('<d', struct.pack('<Q', 0x7FE0000000000000))[0],
                                 struct.unpack('<d', struct.pack('<Q', 0x000FFFFFFFFFFFFF))[0], 1.9999999999999998])
                kw = pack(vw, row, col) & 0xFFFFFFFF      # the winner's low word: any bits above the 11
                nxt = pack_next(vn, kw)
                assert dec(nxt) == (row, col + 1), (row, col)
                assert nxt == pack(vn, row, col + 1), (row, col)
                assert nxt & ~MASK == bits(vn) & ~MASK    # nothing of the value above the 11 bits moves, the high word included


def test_the_add_cannot_carry_out_of_the_eleven_bits():
    # the largest field a consumed key holds is (32 << 5) | 31; + 32 stays below 2^11, and bits above the field that are all
    # ones (a low word of 0xFFFFF800 | field) do not reach it either: the mask drops what the add carries upward
    for row in range(32):
        for col in range(33):
            field = (col << 5) | row
            assert field + 32 <= MASK
            for hi in (0, 0xFFFFF800, 0x80000000):
                assert ((hi | field) + 32) & 0xFFFFFFFF & MASK == ((col + 1) << 5) | row


@pytest.mark.parametrize("NR", LIST_LENGTHS)
def test_weight_table_index_is_unique_and_inside_the_table(NR):
    for G in range(1, NR + 1):
        if G > 1 and any(n >= G for n in LIST_LENGTHS if n < NR):
            continue                                # G runs in the smallest instantiated length >= G
        entries = (G + 1) * 32                      # weight_table_bytes(G) / 8
        seen = set()
        for row in range(G):
            for col in range(G + 1):                # col = G: the key of an exhausted row, read and never used
                idx = (col << 5) | row
                assert idx == pack(1.0, row, col) & MASK
                assert 0 <= idx < entries, (G, row, col)
                assert idx not in seen
                seen.add(idx)
                assert (idx & 31, idx >> 5) == (row, col)
        assert len(seen) == G * (G + 1)


def test_seven_waves_and_the_table_fit_the_lds_at_g20():
    G, tables = 20, (2 * 32 + 2) * 8 + 32 * 4       # DG, GORD, the float32 copy of DG
    shared = tables + (G + 1) * 32 * 8
    rows = (2 * G + 1) * 64 * 8                     # a, b and the sentinel row of one wave
    assert (160 * 1024 - shared) // rows == 7
