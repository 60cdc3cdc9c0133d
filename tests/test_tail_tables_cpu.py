"""The expansion's fragment table of rart_conv3x3_tail_pair staged in LDS (robustart_amd/csrc/conv_tail_pair.hip, TLDS instances) on the
CPU: the library-global tables switch, and the LDS map of the two table buffers.

The table ([256][64]) is stored in MFMA fragment order: fragment f is 1 KiB, lane l's 16 bytes at f * 1024 + 16 l of each plane (hi, lo).
A 64-output-channel chunk c is the 8 fragments 8 c .. 8 c + 7 of both planes: (block b, K step s) -> 8 c + 4 b + s.  A refill is one
rart_dma_load16 per (wave, q, plane): wave w brings fragments k = w and w + 4; lane l's 16 bytes land at
CT_TBL + buf * CT_TBL_BYTES + plane * CT_TBL_PLANE + k * 1024 + 16 l.  A fragment read is a ds_read_b128 at the same expression with
k = 4 b + s.  Chunk c lives in buffer c & 1; chunk c + 1 is issued behind the barrier that publishes chunk c.  Bank model and service
groups: tests/test_stem_pair_bank_model.py."""
import os
import re

from test_stem_pair_bank_model import B128_GROUPS, cycles

# ---- mirrored from conv_tail_pair.hip
CT_NLD = 144
CT_WREG = 2 * 32 * CT_NLD
CT_TBL = 4 * CT_WREG
CT_TBL_PLANE = 8 * 1024
CT_TBL_BYTES = 2 * CT_TBL_PLANE
LDS_BYTES = 79872                                   # 4 slab images + two weight stages (tests/test_tail_slab_cpu.py)
C, NOUT, NC = 64, 256, 4
PLANE_BYTES = NOUT * C * 2                          # one plane of a table in memory: the resources' num_records


def _source():
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'robustart_amd', 'csrc', 'conv_tail_pair.hip')).read()


def refill(chunk, buf):
    """the wave-instructions of one refill -> [(wave, plane, [(source byte offset in the plane, LDS byte address) per lane])]"""
    out = []
    for wave in range(4):
        for q in range(2):
            k = wave + 4 * q
            so = (chunk * 8 + k) * 1024
            la = CT_TBL + buf * CT_TBL_BYTES + k * 1024
            for plane in range(2):
                out.append((wave, plane, [(so + 16 * lane, la + plane * CT_TBL_PLANE + 16 * lane) for lane in range(64)]))
    return out


def read_addr(lane, buf, plane, blk, s):
    return CT_TBL + buf * CT_TBL_BYTES + plane * CT_TBL_PLANE + (blk * 4 + s) * 1024 + 16 * lane


def test_mirrored_constants_and_maps_are_the_kernels():
    src = _source()
    m = re.search(r'constexpr int CT_NLD = (\d+);', src)
    assert m and int(m.group(1)) == CT_NLD
    assert 'constexpr int CT_WREG = 2 * 32 * CT_NLD;' in src
    assert 'constexpr int CT_TBL = 4 * CT_WREG;' in src
    assert 'constexpr int CT_TBL_PLANE = 8 * 1024;' in src
    assert 'constexpr int CT_TBL_BYTES = 2 * CT_TBL_PLANE;' in src
    # the refill, as the kernel writes it
    assert 'const uint32_t tbl_voff = (uint32_t)lane * 16u;' in src
    assert 'const uint32_t k_ = (uint32_t)(wave + 4 * q_);' in src
    assert 'const uint32_t so_ = ((uint32_t)(CHUNK) * 8u + k_) * 1024u;' in src
    assert 'const uint32_t la_ = tbl_lds + (uint32_t)(BUF) * (uint32_t)CT_TBL_BYTES + k_ * 1024u;' in src
    assert 'rart_dma_load16(tbl_voff, srd_th, so_, la_);' in src
    assert 'rart_dma_load16(tbl_voff, srd_tl, so_, la_ + (uint32_t)CT_TBL_PLANE);' in src
    assert 'srd_th[2] = srd_tl[2] = (uint32_t)(NOUT * C * 2);' in src
    # the fragment reads
    assert 'tbuf = lds + CT_TBL + lane * 16 + (c & 1) * CT_TBL_BYTES;' in src
    assert 'th[s] = *reinterpret_cast<const uint4*>(tbuf + (b * KS + sg + s) * 1024);' in src
    assert 'tl[s] = *reinterpret_cast<const uint4*>(tbuf + CT_TBL_PLANE + (b * KS + sg + s) * 1024);' in src
    # which buffer each refill names: chunk 0 before the loop, chunk c + 1 behind the barrier of chunk c
    for line in ('if constexpr (TLDS) { RART_CT_ISSUE_TBL(0, 0) }', 'if (c + 1 < NC) { RART_CT_ISSUE_TBL(c + 1, (c + 1) & 1) }'):
        assert line in src, line
    # one workgroup barrier per chunk, behind the full wait; none anywhere else in the chunk loop
    loop = src[src.index('for (int c = 0; c < NC; ++c) {'):src.index('#undef RART_CT_ISSUE_TBL')]
    assert loop.count('__syncthreads();') == 1 and loop.index('rart_dma_wait<0>();') < loop.index('__syncthreads();') < loop.index('RART_CT_ISSUE_TBL(c + 1')
    assert 'test_tail_tables_cpu.py' in src


def test_table_buffers_lie_behind_the_wave_regions_and_inside_the_allocation():
    bufs = [(CT_TBL + b * CT_TBL_BYTES, CT_TBL + (b + 1) * CT_TBL_BYTES) for b in range(2)]
    waves = [(w * CT_WREG, (w + 1) * CT_WREG) for w in range(4)]
    assert CT_WREG == 9216 and CT_TBL == 36864
    for lo, hi in bufs:
        assert 4 * CT_WREG <= lo < hi <= LDS_BYTES
        assert lo % 256 == 0                                     # a buffer's base moves no bank
        for wlo, whi in waves:
            assert hi <= wlo or whi <= lo
    assert bufs[0][1] <= bufs[1][0]
    # every address a refill writes or a read touches stays inside its buffer
    for buf in range(2):
        for _, _, lanes in refill(3, buf):
            for _, la in lanes:
                assert bufs[buf][0] <= la and la + 16 <= bufs[buf][1]


def test_a_refill_writes_every_slot_once_from_inside_the_table():
    for chunk in range(NC):
        for buf in range(2):
            seen, srcs = {}, set()
            per_wave = [0] * 4
            for wave, plane, lanes in refill(chunk, buf):
                per_wave[wave] += 1
                assert [la for _, la in lanes] == [lanes[0][1] + 16 * l for l in range(64)]      # lane-linear: what the DMA does
                for so, la in lanes:
                    assert 0 <= so and so + 16 <= PLANE_BYTES                                       # inside num_records
                    assert la not in seen
                    seen[la] = (plane, so)
                    srcs.add((plane, so))
            assert per_wave == [4, 4, 4, 4]                                                        # 16 wave-instructions per chunk and table
            assert sorted(seen) == list(range(CT_TBL + buf * CT_TBL_BYTES, CT_TBL + (buf + 1) * CT_TBL_BYTES, 16))
            # the chunk's bytes, all of them, once: fragments 8 c .. 8 c + 7 of both planes
            assert srcs == {(plane, o) for plane in range(2) for o in range(chunk * 8192, (chunk + 1) * 8192, 16)}


def test_fragment_reads_find_the_bytes_the_dma_put_there():
    for chunk in range(NC):
        for buf in range(2):
            where = {}
            for _, plane, lanes in refill(chunk, buf):
                for so, la in lanes:
                    where[la] = (plane, so)
            for plane in range(2):
                for blk in range(2):
                    for s in range(4):
                        for lane in range(64):
                            # th_base[((c * 2 + b) * KS + sg + s) * 64] in uint4 units, + lane
                            want = (((chunk * 2 + blk) * 4 + s) * 64 + lane) * 16
                            assert where[read_addr(lane, buf, plane, blk, s)] == (plane, want)


def test_fragment_reads_are_conflict_free():
    for buf in range(2):
        for plane in range(2):
            for blk in range(2):
                for s in range(4):
                    assert cycles(lambda l: read_addr(l, buf, plane, blk, s), 16, B128_GROUPS) == 4, (buf, plane, blk, s)


def test_tables_switch_refuses_other_values_and_round_trips():
    from robustart_amd import _lib
    lib = _lib.load()
    old = lib.rart_conv3x3_tail_pair_get_tables()
    assert old in (0, 1)
    try:
        for bad in (-1, 2, 7):
            assert lib.rart_conv3x3_tail_pair_set_tables(bad) == 1
            assert b'rart_conv3x3_tail_pair_set_tables' in lib.rart_last_error_string()
            assert lib.rart_conv3x3_tail_pair_get_tables() == old
        for v in (0, 1, 0):
            assert lib.rart_conv3x3_tail_pair_set_tables(v) == 0
            assert lib.rart_conv3x3_tail_pair_get_tables() == v
    finally:
        lib.rart_conv3x3_tail_pair_set_tables(old)
