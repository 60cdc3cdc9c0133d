"""rart_conv3x3_grouped_bf16 / rart_conv3x3_grouped_pair (csrc/conv_grouped.hip) at kernel level against fp64 convolutions of the same
stored operands: forward with bias + ReLU + sign tensor at stride 1 and 2, backward with a 1-bit mask at stride 1 and for the four
input-parity classes at stride 2, every group width, image sizes below / beside / beyond one workgroup tile, the destination inside
non-zero guard bands.  tests/test_grouped_conv_tables_cpu.py shows that these operands make a result with the groups shifted or
ignored miss the same bounds in more than nine outputs of ten.  Each measured error is printed beside its bound (-s)."""
import ctypes

import pytest
import torch

import _grouped_conv_ref as R

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 7.0


def _lib():
    from robustart_amd import _lib as L
    L.require_gpu()
    return L, L.load()


def _tile(lib, gw, split, stride):
    r, c = ctypes.c_int(), ctypes.c_int()
    assert lib.rart_conv3x3_grouped_tile(gw, int(split), stride, ctypes.byref(r), ctypes.byref(c)) == 0
    return r.value, c.value


def _store(x_nchw, split):
    """fp32 NCHW -> device NHWC planes [P][n][h][w][c], P = 1 (bf16) or 2 (hi, lo)"""
    from robustart_amd.model.engine_base import pair
    t = x_nchw.permute(0, 2, 3, 1).contiguous()
    return (pair(t) if split else t.to(torch.bfloat16).unsqueeze(0)).cuda().contiguous()


def _launch(lib, L, split, c, frag, taps, src, grid, dst_shape, stride=1, dst_stride=1, dst_org=(0, 0), bias=None, mask=None, want_sign=False,
            relu=False, gw=None, channels=None):
    """-> (status, value fp64 NCHW, hi plane bf16 NCHW, sign bits bool NCHW or None, guards_ok)"""
    n, dh, dw, C = dst_shape
    numel = n * dh * dw * C
    P = 2 if split else 1
    buf = torch.full((P, numel + 2 * GUARD), FILL, dtype=torch.bfloat16, device='cuda')
    sbuf = torch.full((numel // 8 + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    frag = frag.cuda()
    fr = frag if split else frag.unsqueeze(0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    ty = (ctypes.c_int * 9)(*[t[0] for t in taps])
    tx = (ctypes.c_int * 9)(*[t[1] for t in taps])
    geom = (n, src.shape[2], src.shape[3], channels or C, gw or c.gw, stride, grid[0], grid[1], len(taps), ty, tx, dh, dw, dst_stride,
            dst_org[0], dst_org[1], int(relu), L.stream_ptr())
    b = None if bias is None else bias.cuda()
    m = None if mask is None else R.pack_bits(mask).cuda()
    so = ptr(sbuf[GUARD:]) if want_sign else None
    if split:
        st = lib.rart_conv3x3_grouped_pair(ptr(src[0]), ptr(src[1]), ptr(fr[0]), ptr(fr[1]), L.ptr(b), L.ptr(m), so, ptr(buf[0, GUARD:]),
                                           ptr(buf[1, GUARD:]), *geom)
    else:
        st = lib.rart_conv3x3_grouped_bf16(ptr(src[0]), ptr(fr[0]), L.ptr(b), L.ptr(m), so, ptr(buf[0, GUARD:]), *geom)
    torch.cuda.synchronize()
    host, shost = buf.cpu(), sbuf.cpu()
    guards_ok = bool((host[:, :GUARD] == FILL).all() and (host[:, GUARD + numel:] == FILL).all() and
                     (shost[:GUARD] == 0xA5).all() and (shost[GUARD + numel // 8:] == 0xA5).all())
    if not want_sign:
        guards_ok = guards_ok and bool((shost == 0xA5).all())
    planes = host[:, GUARD:GUARD + numel].reshape(P, n, dh, dw, C).permute(0, 1, 4, 2, 3)
    value = planes[0].double() + (planes[1].double() if split else 0.0)
    sign = R.unpack_bits(shost[GUARD:GUARD + numel // 8], (n, dh, dw, C)) if want_sign else None
    return st, value, planes[0], sign, guards_ok


def _check(tag, got, ref, split):
    err = (got - ref).abs()
    if split:
        bound = R.PAIR_REL * ref.abs().max().item()
        print('%s: max |err| %.3e  bound %.3e (2.5e-5 max |ref|)' % (tag, err.max().item(), bound))
        assert err.max().item() <= bound, tag
    else:
        excess = (err - (ref.abs() * R.BF16_REL + R.BF16_ABS)).max().item()
        print('%s: max |err| %.3e, max (|err| - (|ref| 2^-8 + 1e-6)) %.3e  bound 0' % (tag, err.max().item(), excess))
        assert excess <= 0, tag


def _conv(C, gw, stride, split):
    from robustart_amd.model.engine import _Conv
    conv, bn = R.make_layer(C, gw, stride)
    return _Conv(conv, bn, 'cpu', split)


@pytest.mark.parametrize('split', [False, True], ids=['bf16', 'pair'])
@pytest.mark.parametrize('C,gw', R.CASES)
def test_grouped_forward_bias_relu_sign(C, gw, split):
    L, lib = _lib()
    G = C // gw
    for stride in (1, 2):
        th, tw = _tile(lib, gw, split, stride)
        sizes = [(5, 7), (14, 14), (th + 3, tw + 5)] if stride == 1 else [(8, 12), (14, 14)]
        c = _conv(C, gw, stride, split)
        w, b = R.stored(c.w_folded, split), c.b_folded.double()
        for hw in sizes:
            assert lib.rart_conv3x3_grouped_supported(C, gw, hw[0], hw[1], stride) == 1
            x, _ = R.inputs(C, hw, 11)
            ref = R.ref_forward(R.stored(x, split), w, b, stride, G)
            oh, ow = hw[0] // stride, hw[1] // stride
            st, got, hi, sign, guards = _launch(lib, L, split, c, c.g_fwd[1], c.fwd_taps, _store(x, split), (oh, ow), (R.B, oh, ow, C),
                                                stride=stride, bias=c.bias, want_sign=True, relu=True)
            tag = 'fwd C %d gw %d stride %d %dx%d %s' % (C, gw, stride, hw[0], hw[1], 'pair' if split else 'bf16')
            assert st == 0, L.load().rart_last_error_string()
            _check(tag, got, ref, split)
            assert guards, tag + ': guard bands'
            assert torch.equal(sign, hi.float() > 0), tag + ': sign bits'
            assert 0.5 < sign.float().mean().item() < 0.99 and (got >= 0).all()      # the ReLU clamps, both sign values occur


@pytest.mark.parametrize('split', [False, True], ids=['bf16', 'pair'])
@pytest.mark.parametrize('C,gw', R.CASES)
def test_grouped_backward_masked(C, gw, split):
    L, lib = _lib()
    G = C // gw
    for stride in (1, 2):
        th, tw = _tile(lib, gw, split, 1)         # (every backward launch reads its source at stride 1)
        sizes = [(5, 7), (14, 14), (th + 3, tw + 5)] if stride == 1 else [(8, 12), (14, 14)]
        c = _conv(C, gw, stride, split)
        w = R.stored(c.w_folded, split)
        for hw in sizes:
            oh, ow = hw[0] // stride, hw[1] // stride
            dz, _ = R.inputs(C, (oh, ow), 12)
            _, mask = R.inputs(C, hw, 13)
            ref = R.ref_backward(R.stored(dz, split), w, hw, stride, G, mask)
            src = _store(dz, split)
            for (parity, taps, _), (_, frag) in zip(c.bwd, c.g_bwd):
                tag = 'bwd C %d gw %d stride %d %dx%d class %s %s' % (C, gw, stride, hw[0], hw[1], parity, 'pair' if split else 'bf16')
                if parity is None:
                    st, got, _, _, guards = _launch(lib, L, split, c, frag, taps, src, hw, (R.B, hw[0], hw[1], C), mask=mask)
                    written = torch.ones(hw, dtype=torch.bool)
                else:
                    grid = ((hw[0] - parity[0] + 1) // 2, (hw[1] - parity[1] + 1) // 2)
                    st, got, _, _, guards = _launch(lib, L, split, c, frag, taps, src, grid, (R.B, hw[0], hw[1], C), dst_stride=2,
                                                    dst_org=parity, mask=mask)
                    written = torch.zeros(hw, dtype=torch.bool)
                    written[parity[0]::2, parity[1]::2] = True
                assert st == 0, L.load().rart_last_error_string()
                _check(tag, got[:, :, written], ref[:, :, written], split)
                assert guards, tag + ': guard bands'
                assert (got[:, :, ~written] == FILL * (2 if split else 1)).all(), tag + ': pixels of other classes'


def test_query_and_entries_agree_on_what_is_refused():
    L, lib = _lib()
    c = _conv(64, 8, 1, False)
    x, _ = R.inputs(64, (5, 7), 11)
    src = _store(x, False)
    for channels, gw, stride in ((64, 12, 1), (48, 16, 1), (64, 8, 3), (96, 64, 1), (64, 128, 1), (64, 8, 0)):
        assert lib.rart_conv3x3_grouped_supported(channels, gw, 5, 7, stride) == 0
        st, got, _, _, guards = _launch(lib, L, False, c, c.g_fwd[1], c.fwd_taps, src, (5, 7), (R.B, 5, 7, 64), stride=stride, gw=gw,
                                        channels=channels)
        assert st == 1 and b'unsupported geometry' in lib.rart_last_error_string()
        assert guards and (got == FILL).all()
    # a grid that would leave the destination, taps outside -1 .. 1: refused as well, nothing written
    st, got, _, _, guards = _launch(lib, L, False, c, c.g_fwd[1], c.fwd_taps, src, (5, 7), (R.B, 5, 7, 64), dst_stride=2)
    assert st == 1 and guards and (got == FILL).all()
    st, got, _, _, guards = _launch(lib, L, False, c, c.g_fwd[1], [(2, 0)] * 9, src, (5, 7), (R.B, 5, 7, 64))
    assert st == 1 and guards and (got == FILL).all()
    for gw in (4, 8, 16, 32, 64):
        for stride in (1, 2):
            assert lib.rart_conv3x3_grouped_supported(128, gw, 56, 56, stride) == 1
