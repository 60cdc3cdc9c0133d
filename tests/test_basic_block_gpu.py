"""rart_basic_block_bf16 (csrc/basic_block.hip) at kernel level against fp64 of the same stored operands with the intermediate rounded to
bf16 (tests/test_basic_block_refs_cpu.py holds the references and shows that the bound separates right from wrong):

    |err| <= |ref| 2^-8 + 2 * 2^-8 * max|intermediate| * max|second conv's weights| + 1e-6

forward and backward, n = 3 (image boundaries inside the batch), image sizes around the workgroup tile, every nullable pointer present
and absent, outputs inside guard bands, the conv-by-conv route (two rart_conv_igemm_bf16 launches) held to the same bound, the sign
bits, a poisoned input, and the refused shapes.  Each measured error is printed beside its bound (-s)."""
import ctypes
import functools

import pytest
import torch

import test_basic_block_refs_cpu as R

pytestmark = pytest.mark.gpu
GUARD, FILL, SFILL, N = 64, 7.0, 0xA5, 3
WIDTHS = (64, 128)


def _lib():
    from robustart_amd import _lib as L
    L.require_gpu()
    return L, L.load()


def _tile(lib, c):
    r, w = ctypes.c_int(), ctypes.c_int()
    assert lib.rart_basic_block_tile(c, ctypes.byref(r), ctypes.byref(w)) == 0
    return r.value, w.value


def _sizes(c):
    from robustart_amd import _lib as L
    r, w = _tile(L.load(), c)
    return [(1, 1), (r - 1, w), (r, w), (r + 1, w + 1), (9, 7), (9, 20), (9, 56)]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _pack_bits(m_nchw):
    """bool NCHW -> uint8 [n][h][w][C / 8], bit c % 8 of byte c / 8"""
    m = _nhwc(m_nchw).to(torch.uint8)
    return (m.view(*m.shape[:3], -1, 8) << torch.arange(8, dtype=torch.uint8)).sum(-1).to(torch.uint8).contiguous()


def _unpack_bits(s, shape):
    """uint8 flat -> bool NCHW of NHWC `shape`"""
    b = (s.view(-1, 1) >> torch.arange(8, dtype=torch.uint8)) & 1
    return b.view(shape).bool().permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _case(c, h, w):
    """inputs, references and device tables of one shape, computed once"""
    from robustart_amd.model.engine_base import conv_tap_classes, pad_rows, rows_mult
    L, lib = _lib()
    d = R.make_inputs(c, N, h, w, seed=3 * c + 11 * h + w)
    d['a'], d['mid'], d['out'] = R.ref_forward(d['x'], d['w1'], d['w2'], d['b1'], d['b2'])
    zero = torch.zeros_like(d['b1'])
    d['a0'], d['mid0'], d['out0'] = R.ref_forward(d['x'], d['w1'], d['w2'], zero, zero)
    d['m_mid'], d['m_in'] = d['mid'] > 0, d['x'] > 0
    d['t'], d['dx'] = R.ref_backward(d['g'], d['w1'], d['w2'], d['m_mid'].double(), d['m_in'].double())
    _, d['dx_nomask'] = R.ref_backward(d['g'], d['w1'], d['w2'], d['m_mid'].double(), None)
    fwd_taps, rs, bwd = conv_tap_classes(3, 3, 1, 1)
    d['fwd_taps'], d['bwd_taps'] = fwd_taps, bwd[0][1]
    for k in ('w1', 'w2'):
        wt = d[k]
        rows = {'fwd': torch.cat([wt[:, :, a, b] for a, b in rs], 1), 'bwd': torch.cat([wt[:, :, a, b].t() for a, b in bwd[0][2]], 1)}
        for kind, t in rows.items():
            t = pad_rows(t.to(torch.bfloat16), rows_mult(c)).cuda()
            frag = torch.empty(9 * c * c, dtype=torch.bfloat16, device='cuda')
            assert lib.rart_pack_frag_bf16(L.ptr(t), L.ptr(frag), c, 9 * c, L.stream_ptr()) == 0
            d['%s_%s_rows' % (k, kind)], d['%s_%s_frag' % (k, kind)] = t, frag
    torch.cuda.synchronize()
    return d


class _Out:
    """an output tensor inside guard bands"""

    def __init__(self, numel, dtype, fill):
        self.numel, self.fill = numel, fill
        self.buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device='cuda')

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf[GUARD:].data_ptr())

    def read(self):
        """-> (payload on the host, guards untouched)"""
        h = self.buf.cpu()
        return h[GUARD:GUARD + self.numel], bool((h[:GUARD] == self.fill).all() and (h[GUARD + self.numel:] == self.fill).all())


def _fused(d, c, h, w, backward, x, b1=None, b2=None, m_mid=None, m_io=None, want_mid=False, want_io=False, channels=None, hw=None):
    """one launch -> (status, out fp64 NCHW, raw bf16 NHWC payload, mid sign bool or None, io sign bool or None, guards ok)"""
    L, lib = _lib()
    numel = N * h * w * c
    out, s_mid, s_io = _Out(numel, torch.bfloat16, FILL), _Out(numel // 8, torch.uint8, SFILL), _Out(numel // 8, torch.uint8, SFILL)
    taps = d['bwd_taps'] if backward else d['fwd_taps']
    w1, w2 = (d['w2_bwd_frag'], d['w1_bwd_frag']) if backward else (d['w1_fwd_frag'], d['w2_fwd_frag'])
    ty, tx = (ctypes.c_int * 9)(*[t[0] for t in taps]), (ctypes.c_int * 9)(*[t[1] for t in taps])
    if backward:
        pm, pi = L.ptr(m_mid), L.ptr(m_io)
    else:
        pm, pi = (s_mid.ptr if want_mid else None), (s_io.ptr if want_io else None)
    hh, ww = hw or (h, w)
    st = lib.rart_basic_block_bf16(L.ptr(x), L.ptr(w1), L.ptr(w2), L.ptr(b1), L.ptr(b2), pm, pi, out.ptr, N, hh, ww, channels or c, ty, tx,
                                   int(backward), L.stream_ptr())
    torch.cuda.synchronize()
    o, g0 = out.read()
    sm, g1 = s_mid.read()
    si, g2 = s_io.read()
    if not (want_mid and not backward):
        g1 = g1 and bool((sm == SFILL).all())
    if not (want_io and not backward):
        g2 = g2 and bool((si == SFILL).all())
    shape = (N, h, w, c)
    return (st, o.view(shape).permute(0, 3, 1, 2).double(), o, _unpack_bits(sm, shape) if want_mid else None,
            _unpack_bits(si, shape) if want_io else None, g0 and g1 and g2)


def _igemm(L, lib, src, rows, dst, c, h, w, taps, **kw):
    from robustart_amd.model.engine_base import conv_desc
    desc = conv_desc(src, rows, dst, N, (h, w), (h, w), c, c, taps, c, (h, w), c, **kw)
    assert lib.rart_conv_igemm_bf16(ctypes.byref(desc), L.stream_ptr()) == 0, lib.rart_last_error_string()


def _unfused(d, c, h, w, backward, x, b1, b2, m_mid_bits, m_in_bits):
    """the conv-by-conv route: two implicit-GEMM launches, the intermediate stored in bf16 -> out fp64 NCHW"""
    from robustart_amd.model.engine_base import F_MASK_BITS, F_RELU
    L, lib = _lib()
    shape = (N, h, w, c)
    mid = torch.empty(shape, dtype=torch.bfloat16, device='cuda')
    out = torch.empty(shape, dtype=torch.bfloat16, device='cuda')
    if not backward:
        _igemm(L, lib, x, d['w1_fwd_rows'], mid, c, h, w, d['fwd_taps'], bias=b1, flags=F_RELU)
        _igemm(L, lib, mid, d['w2_fwd_rows'], out, c, h, w, d['fwd_taps'], bias=b2, res=x, flags=F_RELU)
    else:
        _igemm(L, lib, x, d['w2_bwd_rows'], mid, c, h, w, d['bwd_taps'], mask=m_mid_bits, flags=F_MASK_BITS)
        _igemm(L, lib, mid, d['w1_bwd_rows'], out, c, h, w, d['bwd_taps'], res=x, mask=m_in_bits, flags=F_MASK_BITS)
    torch.cuda.synchronize()
    return out.cpu().permute(0, 3, 1, 2).double()


def _check(tag, got, ref, mid, w_second):
    err, bnd = (got - ref).abs(), R.bound(ref, mid, w_second)
    worst = (err / bnd).max().item()
    print('%s: max |err| %.3e, worst |err| / bound %.3f  (bound <= 1)' % (tag, err.max().item(), worst))
    assert worst <= 1.0, tag


CASES = [(c, h, w) for c in WIDTHS for h, w in _sizes(c)]


@pytest.mark.parametrize('c,h,w', CASES, ids=['%d@%dx%d' % k for k in CASES])
def test_forward(c, h, w):
    L, lib = _lib()
    assert lib.rart_basic_block_supported(c, h, w) == 1
    d = _case(c, h, w)
    tag = 'fwd %d@%dx%d' % (c, h, w)
    x = _nhwc(d['x']).to(torch.bfloat16).cuda()
    b1, b2 = d['b1'].float().cuda(), d['b2'].float().cuda()
    st, got, raw, s_mid, s_io, guards = _fused(d, c, h, w, False, x, b1, b2, want_mid=True, want_io=True)
    assert st == 0, lib.rart_last_error_string()
    _check(tag + ' fused', got, d['out'], d['mid'], d['w2'])
    assert guards, tag + ': guard bands'
    _check(tag + ' conv by conv', _unfused(d, c, h, w, False, x, b1, b2, None, None), d['out'], d['mid'], d['w2'])
    # sign bits: out's are exact against the stored values, the intermediate's against the fp64 sign away from zero
    assert torch.equal(s_io, got > 0), tag + ': sign bits of out'
    a = d['a']
    sure = a.abs() >= 1e-4 * a.abs().max()
    print('%s: %.3f %% of the intermediates excluded from the sign comparison (allowed 0.2 %%)' % (tag, 100 * (1 - sure.double().mean().item())))
    assert (1 - sure.double().mean().item()) <= 0.002
    assert torch.equal(s_mid[sure], (a > 0)[sure]), tag + ': sign bits of the intermediate'
    # every nullable pointer absent in turn: the same stored values, the remaining outputs unchanged
    for wm, wi in ((False, True), (True, False), (False, False)):
        st, _, raw2, s2m, s2i, g2 = _fused(d, c, h, w, False, x, b1, b2, want_mid=wm, want_io=wi)
        assert st == 0 and g2 and torch.equal(raw2.view(torch.int16), raw.view(torch.int16)), tag + ': nullable sign pointers'
        assert (s2m is None or torch.equal(s2m, s_mid)) and (s2i is None or torch.equal(s2i, s_io))
    st, got0, _, _, _, g0 = _fused(d, c, h, w, False, x, None, None)
    assert st == 0 and g0
    _check(tag + ' fused, no biases', got0, d['out0'], d['mid0'], d['w2'])


@pytest.mark.parametrize('c,h,w', CASES, ids=['%d@%dx%d' % k for k in CASES])
def test_backward(c, h, w):
    L, lib = _lib()
    d = _case(c, h, w)
    tag = 'bwd %d@%dx%d' % (c, h, w)
    g = _nhwc(d['g']).to(torch.bfloat16).cuda()
    m_mid, m_in = _pack_bits(d['m_mid']).cuda(), _pack_bits(d['m_in']).cuda()
    st, got, _, _, _, guards = _fused(d, c, h, w, True, g, m_mid=m_mid, m_io=m_in)
    assert st == 0, lib.rart_last_error_string()
    _check(tag + ' fused', got, d['dx'], d['t'], d['w1'])
    assert guards, tag + ': guard bands'
    _check(tag + ' conv by conv', _unfused(d, c, h, w, True, g, None, None, m_mid, m_in), d['dx'], d['t'], d['w1'])
    st, got, _, _, _, guards = _fused(d, c, h, w, True, g, m_mid=m_mid, m_io=None)
    assert st == 0 and guards
    _check(tag + ' fused, no m_in', got, d['dx_nomask'], d['t'], d['w1'])
    assert (got != 0).double().mean().item() > 0.5          # nothing masked the result


def test_nan_and_inf_reach_the_outputs_that_read_them_and_no_others():
    L, lib = _lib()
    c = 64
    r, tw = _tile(lib, c)
    h, w = r + 1, tw + 1
    d = _case(c, h, w)
    b1, b2 = d['b1'].float().cuda(), d['b2'].float().cuda()
    x = _nhwc(d['x']).to(torch.bfloat16)
    st, _, clean, _, _, _ = _fused(d, c, h, w, False, x.cuda(), b1, b2)
    assert st == 0
    bad = x.clone()
    ny, nx, iy, ix = r - 1, 3, 0, w - 1            # the NaN beside a tile edge of image 0, the +Inf in a corner of image 1
    bad[0, ny, nx, 5] = float('nan')
    bad[1, iy, ix, 9] = float('inf')
    st, got, raw, _, _, guards = _fused(d, c, h, w, False, bad.cuda(), b1, b2)
    assert st == 0 and guards
    near = torch.zeros(N, h, w, dtype=torch.bool)
    near[0, max(ny - 2, 0):ny + 3, max(nx - 2, 0):nx + 3] = True
    nan_zone = near.clone()
    near[1, max(iy - 2, 0):iy + 3, max(ix - 2, 0):ix + 3] = True
    raw, clean = raw.view(N, h, w, c), clean.view(N, h, w, c)
    assert torch.equal(raw[~near].view(torch.int16), clean[~near].view(torch.int16)), 'a poisoned pixel changed an output that does not read it'
    assert torch.isnan(raw[nan_zone]).all(), 'the NaN did not reach every output that reads it'
    assert not torch.isfinite(raw[1, iy, ix, 9]), 'the +Inf did not reach its own output'
    print('NaN: all %d outputs of its 5 x 5 neighbourhood are NaN; %d outputs elsewhere are bit-identical to the clean run'
          % (int(nan_zone.sum()) * c, int((~near).sum()) * c))


def test_query_and_entry_agree_on_refused_shapes_and_a_refused_call_writes_nothing():
    L, lib = _lib()
    c, h, w = 64, 9, 7
    d = _case(c, h, w)
    x = _nhwc(d['x']).to(torch.bfloat16).cuda()
    for ch, hh, ww in ((32, 9, 7), (96, 9, 7), (256, 14, 14), (512, 7, 7), (64, 0, 7), (64, 9, 0), (128, -1, 4)):
        assert lib.rart_basic_block_supported(ch, hh, ww) == 0
        st, _, raw, _, _, guards = _fused(d, c, h, w, False, x, channels=ch, hw=(hh, ww), want_mid=False, want_io=False)
        assert st == 1 and guards and bool((raw == FILL).all()), (ch, hh, ww)
    for ch in WIDTHS:
        for hh, ww in ((1, 1), (9, 7), (56, 56), (300, 500)):
            assert lib.rart_basic_block_supported(ch, hh, ww) == 1
