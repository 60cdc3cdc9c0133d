"""The input slab of rart_conv3x3_tail_pair (robustart_amd/csrc/conv_tail_pair.hip, SLAB instances) on the CPU: the library-global
staging switch, the LDS bank model of the slab's fragment reads, and the write map of a slab piece.

The slab is four images [K half][hi / lo] of CT_SLAB_ROWS rows x 64 B.  A 1 KiB piece is 16 rows; lane l of the loading wave writes
bytes 16 l .. 16 l + 15 of the piece: row-in-piece l >> 2, LDS chunk l & 3, which receives the row's source chunk (l & 3) ^ ((row >> 2) & 3).
A fragment read of tap t takes slab row R = 32 wave + fr + (dy_t + 1) W + (dx_t + 1) (fr = lane & 31, h = lane >> 5) and, for K sub-step
ks, source chunk 2 ks + h, i.e. byte R * 64 + (((2 ks + h) ^ ((R >> 2) & 3)) << 4) of the image.  Bank model and service groups:
tests/test_stem_pair_bank_model.py."""
import os
import re

from test_stem_pair_bank_model import B128_GROUPS, cycles

# ---- mirrored from conv_tail_pair.hip
CT_TM = 128
CT_SLAB_ROWS = 248
CT_SLAB_IMG = CT_SLAB_ROWS * 64
W_MAX = (CT_SLAB_ROWS - CT_TM) // 2 - 1          # the widest row the launcher sends to the slab path


def _source():
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'robustart_amd', 'csrc', 'conv_tail_pair.hip')).read()


def read_addr(lane, row_off, ks, image):
    fr, h = lane & 31, lane >> 5
    R = row_off + fr
    return image * CT_SLAB_IMG + R * 64 + (((2 * ks + h) ^ ((R >> 2) & 3)) << 4)


def write_map(piece):
    """lane -> (LDS byte offset in the image, slab row, source chunk) of one piece"""
    out = []
    for lane in range(64):
        row = 16 * piece + (lane >> 2)
        out.append((piece * 1024 + 16 * lane, row, (lane & 3) ^ ((lane >> 4) & 3)))
    return out


def test_mirrored_constants_and_maps_are_the_kernels():
    src = _source()
    for name, val in (('CT_TM', CT_TM), ('CT_SLAB_ROWS', CT_SLAB_ROWS)):
        m = re.search(r'constexpr int %s = (\d+);' % name, src)
        assert m and int(m.group(1)) == val, name
    assert 'constexpr int CT_SLAB_IMG = CT_SLAB_ROWS * 64;' in src
    # the lane maps mirrored above, as the kernel writes them
    assert 'lane_off = (uint32_t)((((lane & 3) ^ ((lane >> 4) & 3)) << 4))' in src
    assert 'const int srow = 16 * piece + (lane >> 2);' in src
    assert 'so[ks] = (uint32_t)(R * 64 + (((2 * ks + h) ^ ((R >> 2) & 3)) << 4));' in src
    assert 'const int rbase = wave * 32 + fr + halo;' in src
    assert 'CT_TM + 2 * (t->w + 1) <= CT_SLAB_ROWS' in src
    assert 'test_tail_slab_cpu.py' in src
    assert W_MAX == 59 and CT_TM + 2 * (W_MAX + 1) <= CT_SLAB_ROWS < CT_TM + 2 * (W_MAX + 2)
    # the images are whole multiples of the 256-byte bank period, so an image's base moves no bank
    assert CT_SLAB_IMG % 256 == 0 and 4 * CT_SLAB_IMG + 16384 == 79872


def test_slab_fragment_reads_are_conflict_free():
    """4 cycles per ds_read_b128 for every row offset the kernel can produce: the wave bases 0 / 32 / 64 / 96 plus (dy + 1) W + (dx + 1)
    = 0 .. 2 W_MAX + 2, both K sub-steps, every image."""
    n = 0
    for wave in range(4):
        for tap_off in range(0, 2 * W_MAX + 3):
            row_off = 32 * wave + tap_off
            assert row_off + 31 < CT_SLAB_ROWS
            for ks in range(2):
                for image in range(4):
                    assert cycles(lambda l: read_addr(l, row_off, ks, image), 16, B128_GROUPS) == 4, (wave, tap_off, ks, image)
                    n += 1
    assert n == 4 * (2 * W_MAX + 3) * 2 * 4


def test_a_piece_fills_its_kib_exactly_once_and_reads_find_their_chunk():
    pieces = (CT_SLAB_ROWS + 15) // 16
    where = {}
    for piece in range(pieces):
        wm = write_map(piece)
        covered = sorted(off - piece * 1024 for off, _, _ in wm)
        assert covered == list(range(0, 1024, 16))                       # 64 lanes x 16 B: every 16-byte slot of the KiB once
        for off, row, chunk in wm:
            assert (row, chunk) not in where
            where[(row, chunk)] = off
    # the last piece has 8 rows: the lanes the kernel keeps out of the load are exactly those past the slab
    last = [row for _, row, _ in write_map(pieces - 1)]
    assert [r < CT_SLAB_ROWS for r in last] == [lane < 32 for lane in range(64)]
    assert max(off for (row, _), off in where.items() if row < CT_SLAB_ROWS) + 16 == CT_SLAB_IMG
    # a fragment read of (row, source chunk) lands on the bytes the loader put that chunk in
    for row in range(CT_SLAB_ROWS):
        for ks in range(2):
            for h in range(2):
                lane = (row & 31) | (h << 5)
                assert read_addr(lane, row - (row & 31), ks, 0) == where[(row, 2 * ks + h)]


def test_staging_switch_refuses_other_values_and_round_trips():
    from robustart_amd import _lib
    lib = _lib.load()
    old = lib.rart_conv3x3_tail_pair_get_staging()
    assert old in (0, 1)
    try:
        for bad in (-1, 2, 7):
            assert lib.rart_conv3x3_tail_pair_set_staging(bad) == 1
            assert b'rart_conv3x3_tail_pair_set_staging' in lib.rart_last_error_string()
            assert lib.rart_conv3x3_tail_pair_get_staging() == old
        for v in (0, 1, 0):
            assert lib.rart_conv3x3_tail_pair_set_staging(v) == 0
            assert lib.rart_conv3x3_tail_pair_get_staging() == v
    finally:
        lib.rart_conv3x3_tail_pair_set_staging(old)
