"""LDS bank model of the fragment reads of the two fused reference-precision stem kernels (robustart_amd/csrc/stem_pair.hip), on the CPU.

gfx950 services a wave64 LDS read in fixed lane groups, one LDS cycle per group when no two lanes of the group need different
addresses on one of the 64 four-byte banks (equal addresses broadcast): ds_read_b128 in four groups of 16 lanes
{0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32; ds_read_b64 in the two halves of the wave.  Conflict free is therefore
4 cycles per ds_read_b128 and 2 per ds_read_b64.  The kernel's constants and lane -> address maps are mirrored below (and compared with
the source text, so the mirror cannot drift); every fragment read they produce must cost the conflict-free count:
  forward   A fragments of the patch over all 10 M tiles, 7 row taps, 2 K steps, both planes
  backward  A fragments of the halo tile over the 4 waves, 7 halo rows, 4 dq; the pooled-gradient (16 B) and argmax-code (8 B) reads of
            the pool backward over the four parity classes
`cycles` also refuses an address off the natural alignment of its read (a misaligned 16-byte read is split or replayed by the hardware; its cost is not part of this model).
The layouts before this test existed failed it: 7.17 cycles per forward A read (patch rows of 40 pixels), 7.6-10.0 per
pooled-gradient read and 3.7-3.8 per code read (chunk-major planes of 121 windows)."""
import os
import re

B128_GROUPS = [[l + o for l in g] for o in (0, 32) for g in
               (list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)))]
B64_GROUPS = [list(range(0, 32)), list(range(32, 64))]

# ---- mirrored from stem_pair.hip
SP_PT, SP_PW, SP_ODD, SP_NT = 8, 49, 400, 3
SP_R = 2 * SP_PT + 1
SP_NPOS = SP_R * SP_R
SP_PH = 2 * (SP_R - 1) + 7
SP_PLANE = (SP_PH + 1) // 2 * SP_PW * 16


def sp_row_off(row):
    return (row >> 1) * (SP_PW * 16) + (row & 1) * SP_ODD


T, PTS, NPOS_PAD = 16, 12, 368
HT = T + 3
PT = T // 2 + 3
NPOOL_PAD = PT * PTS


def cycles(addr_of_lane, nbytes, groups, per_group=False):
    """LDS cycles of one wave-instruction; addr_of_lane(lane) -> byte address, or None for a lane that is masked off.  With
    per_group the worst single group instead (1 = no conflict, whatever lanes are masked off)."""
    total, worst = 0, 0
    for grp in groups:
        banks = {}
        for lane in grp:
            a = addr_of_lane(lane)
            if a is None:
                continue
            assert a % nbytes == 0
            for d in range(a // 4, (a + nbytes) // 4):
                banks.setdefault(d % 64, set()).add(d)
        n = max((len(v) for v in banks.values()), default=0)
        total, worst = total + n, max(worst, n)
    return worst if per_group else total


def test_mirrored_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'robustart_amd', 'csrc', 'stem_pair.hip')).read()
    for name, val in (('SP_PT', SP_PT), ('SP_PW', SP_PW), ('SP_ODD', SP_ODD), ('SP_NT', SP_NT), ('T', T), ('PTS', PTS), ('NPOS_PAD', NPOS_PAD)):
        m = re.search(r'constexpr int %s = (\d+);' % name, src)
        assert m and int(m.group(1)) == val, name
    assert 'test_stem_pair_bank_model.py' in src


def test_forward_a_fragment_reads_are_conflict_free():
    worst, n = 0, 0
    for wm in range(4):
        mt0 = wm * SP_NT if wm < 2 else 2 * SP_NT + (wm - 2) * (SP_NT - 1)
        for i in range(SP_NT if wm < 2 else SP_NT - 1):
            def a_off(lane, mt0=mt0, i=i):
                p = min((mt0 + i) * 32 + (lane & 31), SP_NPOS - 1)
                py, px = divmod(p, SP_R)
                return py * (SP_PW * 16) + 2 * px * 8 + (lane >> 5) * 16
            for r in range(7):
                for ks in range(2):
                    for plane in (0, SP_PLANE):
                        c = cycles(lambda l: a_off(l) + plane + sp_row_off(r) + ks * 32, 16, B128_GROUPS)
                        worst, n = max(worst, c), n + 1
    assert n == 10 * 7 * 2 * 2
    assert worst == 4


def test_backward_a_fragment_reads_are_conflict_free():
    for wave in range(4):
        for r in range(7):
            for dqi in range(4):
                for plane in (0, 4):
                    c = cycles(lambda l: ((plane + (l >> 4)) * NPOS_PAD + (wave * 4 + r) * HT + (l & 15) + dqi) * 16, 16, B128_GROUPS)
                    assert c == 4


def _pool_bwd_reads(ey, ex):
    """the wave-instructions of pool_bwd_class_pair<EY, EX> on an interior tile -> [(lane -> window slot lp or None)] per
    (loop pass, wave, window of the position)"""
    ny = (HT + 1) // 2 if ey else HT // 2
    nx = (HT + 1) // 2 if ex else HT // 2
    out = []
    n_iter = (4 * ny * PTS + 31) & ~31
    for first in range(0, n_iter, 256):
        for wave in range(4):
            for ia in range(2 if ey else 1):
                for ib in range(2 if ex else 1):
                    def slot(lane, first=first, wave=wave, ia=ia, ib=ib):
                        i = first + wave * 64 + lane
                        if i >= n_iter:
                            return None
                        c, j = (i >> 3) & 3, (i & 7) + ((i >> 5) << 3)
                        iy, ix = divmod(j, PTS)
                        if iy >= ny or ix >= nx:
                            return None
                        hy, hx = 2 * iy + (0 if ey else 1), 2 * ix + (0 if ex else 1)
                        # tile origin (a0, b0) = (0, 0): py = hy - 1, qy0 = -1, so qy - qy0 = (py >> 1) + ia + 1
                        ry, rx = ((hy - 1) >> 1) + ia + 1, ((hx - 1) >> 1) + ib + 1
                        assert 0 <= ry < PT and 0 <= rx < PT
                        return (ry * PTS + rx) * 4 + c
                    if any(slot(l) is not None for l in range(64)):
                        out.append(slot)
    return out


def test_pool_backward_reads_are_conflict_free():
    for ey in (0, 1):
        for ex in (0, 1):
            reads = _pool_bwd_reads(ey, ex)
            assert reads
            for slot in reads:
                scaled = lambda l, k: None if slot(l) is None else slot(l) * k      # noqa: E731
                for plane in (0, NPOOL_PAD * 4 * 16):                             # sDp, 16 bytes per (window, chunk), hi and lo plane
                    assert cycles(lambda l: None if slot(l) is None else slot(l) * 16 + plane, 16, B128_GROUPS, True) == 1
                assert cycles(lambda l: scaled(l, 8), 8, B64_GROUPS, True) == 1          # sArg, 8 bytes per (window, chunk)
            # (a partly masked wave can cost less than a full one, never more:) the full waves cost the conflict-free count
            assert max(cycles(lambda l: None if s(l) is None else s(l) * 16, 16, B128_GROUPS) for s in reads) == 4
            assert max(cycles(lambda l: None if s(l) is None else s(l) * 8, 8, B64_GROUPS) for s in reads) == 2
