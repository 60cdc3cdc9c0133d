"""Reference-precision ResNet-50: layer1 block 0's conv1 (1x1, 64 -> 64) + bias + ReLU inside the fused stem forward.

rart_engine_stem_fwd_next_pair against the two launches it replaces -- rart_engine_stem_fwd_fused_pair, then rart_gemm_pair_bf16 on the
pooled pair (one tap, K = 64, bias, ReLU, sign bits): the pooled pair, the argmax codes and both sign tensors unchanged, conv1's output
pair and its sign bits equal bit for bit (the same products in the same order on the same rounded pair).  The engine switch
`fused_stem_next_pair` moves no bit of the logits or of the input gradient."""
import ctypes

import pytest
import torch

gpu = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _split(t):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


@gpu
@pytest.mark.parametrize('u8,H,W', [(False, 64, 64), (True, 64, 64),
                                    (False, 72, 88)])      # pooled 18 x 22: ragged 8 x 8 tiles (sizes the engine never takes)
def test_stem_next_equals_the_separate_launch(u8, H, W):
    from robustart_amd import _lib
    from robustart_amd.model.engine_base import stem_rows
    lib = _lib.load()
    g = torch.Generator().manual_seed(7 + u8 + H)
    B = 2
    wb = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    wf = _split(stem_rows(wb)).cuda()
    bias = (torch.randn(64, generator=g) * 0.2).cuda()
    w1 = _split((torch.randn(64, 64, generator=g) * 0.125).cuda())
    tab = torch.cat([w1[0], w1[1], w1[0]], 1).contiguous()               # the engine's [hi | lo | hi] rows: ldw = 192
    b1 = (torch.randn(64, generator=g) * 0.3).cuda()
    if u8:
        src = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    else:
        src = torch.rand(B, 3, H, W, generator=g).cuda()
    h2, w2 = H // 4, W // 4
    m3, s3 = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    sp = _lib.stream_ptr()

    def outs():
        return (torch.full((2, B, h2, w2, 64), float('nan'), dtype=torch.bfloat16, device='cuda'),
                torch.full((B, h2, w2, 64), 0xEE, dtype=torch.uint8, device='cuda'), torch.full((B, h2, w2, 8), 0xEE, dtype=torch.uint8, device='cuda'))
    p1, arg, sign = outs()
    _lib.check(lib.rart_engine_stem_fwd_fused_pair(_lib.ptr(src), int(u8), _lib.ptr(wf[0]), _lib.ptr(wf[1]), _lib.ptr(bias), _lib.ptr(p1[0]),
                                                   _lib.ptr(p1[1]), _lib.ptr(arg), _lib.ptr(sign), B, H, W, m3, s3, sp))
    want = torch.full((2, B, h2, w2, 64), float('nan'), dtype=torch.bfloat16, device='cuda')
    want_sign = torch.full((B, h2, w2, 8), 0xEE, dtype=torch.uint8, device='cuda')
    d = _lib.GemmPairDesc()
    d.a_hi, d.a_lo, d.w_hi, d.w_lo = p1[0].data_ptr(), p1[1].data_ptr(), tab.data_ptr(), tab.data_ptr() + 2 * 64
    d.bias, d.dst_hi, d.dst_lo, d.sign_out, d.flags = b1.data_ptr(), want[0].data_ptr(), want[1].data_ptr(), want_sign.data_ptr(), 1
    d.N, d.lda, d.ldw, d.ldc, d.w_rows = 64, 64, 192, 64, 64
    d.conv, d.batch, d.grid_h, d.grid_w, d.src_h, d.src_w, d.sy, d.sx, d.k_per_tap, d.n_taps = 1, B, h2, w2, h2, w2, 1, 1, 64, 1
    d.dst_h, d.dst_w, d.dst_sy, d.dst_sx = h2, w2, 1, 1
    _lib.check(lib.rart_gemm_pair_bf16(ctypes.byref(d), sp))
    p1n, argn, signn = outs()
    got = torch.full((2, B, h2, w2, 64), float('nan'), dtype=torch.bfloat16, device='cuda')
    got_sign = torch.full((B, h2, w2, 8), 0xEE, dtype=torch.uint8, device='cuda')
    _lib.check(lib.rart_engine_stem_fwd_next_pair(_lib.ptr(src), int(u8), _lib.ptr(wf[0]), _lib.ptr(wf[1]), _lib.ptr(bias), _lib.ptr(p1n[0]),
                                                  _lib.ptr(p1n[1]), _lib.ptr(argn), _lib.ptr(signn), ctypes.c_void_p(tab.data_ptr()),
                                                  ctypes.c_void_p(tab.data_ptr() + 2 * 64), 192, _lib.ptr(b1), _lib.ptr(got[0]), _lib.ptr(got[1]),
                                                  _lib.ptr(got_sign), B, H, W, m3, s3, sp))
    torch.cuda.synchronize()
    assert torch.isfinite(p1.float()).all() and torch.isfinite(want.float()).all() and torch.isfinite(got.float()).all()
    assert torch.equal(p1n.view(torch.int16), p1.view(torch.int16)) and torch.equal(argn, arg) and torch.equal(signn, sign)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(got_sign, want_sign)
    assert (want[0] > 0).any() and (want[0] == 0).any()                  # the ReLU is exercised both ways
    # the next 1x1 needs both table planes and both output planes
    assert lib.rart_engine_stem_fwd_next_pair(_lib.ptr(src), int(u8), _lib.ptr(wf[0]), _lib.ptr(wf[1]), _lib.ptr(bias), _lib.ptr(p1n[0]),
                                              _lib.ptr(p1n[1]), _lib.ptr(argn), _lib.ptr(signn), ctypes.c_void_p(tab.data_ptr()), None, 192,
                                              _lib.ptr(b1), _lib.ptr(got[0]), _lib.ptr(got[1]), _lib.ptr(got_sign), B, H, W, m3, s3, sp) != 0


@gpu
def test_x3_stem_next_moves_no_bit():
    """Full ResNet-50 at B = 2, 64 x 64, fp32 and uint8 sources: `fused_stem_next_pair` on against off -- logits and input gradient bit-equal,
    one pair launch fewer, block 0's conv1 output and sign tensor the same buffers with the same bits."""
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    torch.manual_seed(0)
    m = randomize_bn_stats(get_model({'type': 'resnet50_official'}), 0).eval().cuda()
    for p in m.parameters():
        p.requires_grad_(False)
    eng = ResNet50Engine(m, 'cuda', precision='fp32x')
    g = torch.Generator().manual_seed(44)
    x = torch.rand(2, 3, 64, 64, generator=g).cuda()
    y = torch.randint(0, 1000, (2,), generator=g).cuda()
    assert eng.fused_stem_next_pair and 'u8' in eng.fused_stem_next_sources
    eng.fused_stem_next_sources = ('u8', 'f32')          # (the engine folds for uint8 sources only, by measurement: both forms are checked here)

    def run():
        n = [0]
        real = eng._launch_pair
        eng._launch_pair = lambda d, nbytes=None: (n.__setitem__(0, n[0] + 1), real(d, nbytes))[1]
        try:
            lo, _, gr, _ = eng.forward_backward(x, MEAN, STD, y, 0)
        finally:
            del eng._launch_pair
        return lo.clone(), gr.clone(), eng._buf['b0_a'].clone(), eng._buf['b0_a_sign'].clone(), n[0]
    la, ga, ya, sa, na = run()
    eng.fused_stem_next_pair = False
    try:
        lb, gb, yb, sb, nb = run()
    finally:
        eng.fused_stem_next_pair = True
    assert nb == na + 1
    assert torch.equal(ya.view(torch.int16), yb.view(torch.int16)) and torch.equal(sa, sb)
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    xu = (x.permute(0, 2, 3, 1) * 255).round().to(torch.uint8).contiguous()
    lu = eng.logits_from_u8(xu, MEAN, STD).clone()
    eng.fused_stem_next_pair = False
    try:
        assert torch.equal(eng.logits_from_u8(xu, MEAN, STD), lu)
    finally:
        eng.fused_stem_next_pair = True
