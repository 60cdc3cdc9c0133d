"""rart_conv3x3_tail_pair with the 3x3's input staged once per tile (the slab, staging 1) against the same launch staged per tap
(staging 0): the slab path runs the same products in the same order, so every output is compared with torch.equal -- the pair the kernel
writes, the neighbour's reduction, and the three sign tensors.

Geometries (C = 64, the only width the slab serves), the smallest that exercise each way the slab can go wrong:
  2 x 9 x 11   a 128-position tile spans two images; M = 198 is no multiple of 128
  1 x 5 x 59   the widest row the slab serves: three tiles, and the last slab runs past the end of the plane
  3 x 4 x 4    images smaller than the taps' reach: one slab covers several images
  1 x 3 x 60   one column too wide: the launch must keep per-tap staging under staging 1, and still be equal
The input planes are separate allocations of exactly M x 64 elements; every output buffer starts as NaN (sign tensors as 0xAA) and must come
back finite."""
import ctypes

import pytest
import torch

gpu = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
C = 64
N = 4 * C

GEOMETRIES = [(2, 9, 11), (1, 5, 59), (3, 4, 4), (1, 3, 60)]
MODES = ['fwd', 'bwd', 'fwd_next', 'bwd_next', 'xs', 'xs_next']


def _split(t):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


def _case(_lib, mode, B, H, W):
    """-> (descriptor, {name: output tensor}, tensors to keep alive)"""
    g = torch.Generator().manual_seed(1000 * B + 10 * W + len(mode))
    P = B * H * W
    backward, nxt, xs = mode.startswith('bwd'), mode.endswith('next'), mode.startswith('xs')
    a = torch.randn(B, H, W, C, generator=g)
    a_hi = a.to(torch.bfloat16).cuda()                               # two allocations of exactly P x 64 elements: no slack after a plane
    a_lo = (a - a.to(torch.bfloat16).float()).to(torch.bfloat16).cuda()
    w2p = _split((torch.randn(C, 9 * C, generator=g) * (2.0 / (9 * C)) ** 0.5).cuda())
    tab = torch.cat([w2p[0], w2p[1], w2p[0]], 1).contiguous()
    frag = lambda p: torch.stack([p[pl].reshape(N // 32, 32, C // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)    # noqa: E731
                                  for pl in range(2)]).contiguous()
    tail = frag(_split((torch.randn(N, C, generator=g) * (1.0 / C) ** 0.5).cuda()))
    keep = [a_hi, a_lo, tab, tail]
    out = {'dst': torch.full((2, P, N), float('nan'), dtype=torch.bfloat16, device='cuda')}
    d = _lib.ConvTailDesc()
    d.a_hi, d.a_lo, d.w_hi, d.w_lo = a_hi.data_ptr(), a_lo.data_ptr(), tab.data_ptr(), tab.data_ptr() + 2 * 9 * C
    d.t_hi, d.t_lo, d.dst_hi, d.dst_lo = tail[0].data_ptr(), tail[1].data_ptr(), out['dst'][0].data_ptr(), out['dst'][1].data_ptr()
    d.batch, d.h, d.w, d.c_mid, d.ldw = B, H, W, C, 3 * 9 * C
    for i in range(9):
        d.tap_dy[i], d.tap_dx[i] = (1 - i // 3, 1 - i % 3) if backward else (i // 3 - 1, i % 3 - 1)      # backward: the flipped taps
    if xs:
        x = _split(torch.randn(P, C, generator=g).cuda())
        tx = frag(_split((torch.randn(N, C, generator=g) * (1.0 / C) ** 0.5).cuda()))
        keep += [x, tx]
        d.x_hi, d.x_lo, d.tx_hi, d.tx_lo = x[0].data_ptr(), x[1].data_ptr(), tx[0].data_ptr(), tx[1].data_ptr()
    else:
        res = _split(torch.randn(P, N, generator=g).cuda())
        keep.append(res)
        d.res_hi, d.res_lo = res[0].data_ptr(), res[1].data_ptr()
    if backward:
        mm = torch.randint(0, 256, (P, C // 8), generator=g, dtype=torch.uint8).cuda()
        mo = torch.randint(0, 256, (P, N // 8), generator=g, dtype=torch.uint8).cuda()
        keep += [mm, mo]
        d.mask_mid, d.mask_out = mm.data_ptr(), mo.data_ptr()
    else:
        b2, b3 = torch.randn(C, generator=g).cuda() * 0.3, torch.randn(N, generator=g).cuda() * 0.3
        keep += [b2, b3]
        out['sign_mid'] = torch.full((P, C // 8), 0xAA, dtype=torch.uint8, device='cuda')
        out['sign_out'] = torch.full((P, N // 8), 0xAA, dtype=torch.uint8, device='cuda')
        d.bias_mid, d.bias_out, d.sign_mid, d.sign_out = b2.data_ptr(), b3.data_ptr(), out['sign_mid'].data_ptr(), out['sign_out'].data_ptr()
        d.relu_mid = d.relu_out = 1
    if nxt:
        wnp = _split((torch.randn(C, N, generator=g) * (1.0 / N) ** 0.5).cuda())
        ntab = torch.stack([wnp[pl].reshape(C // 32, 32, N // 64, 4, 2, 8).permute(2, 0, 3, 4, 1, 5).contiguous().view(-1)
                            for pl in range(2)]).contiguous()
        keep.append(ntab)
        out['dstn'] = torch.full((2, P, C), float('nan'), dtype=torch.bfloat16, device='cuda')
        d.n_hi, d.n_lo, d.dstn_hi, d.dstn_lo = ntab[0].data_ptr(), ntab[1].data_ptr(), out['dstn'][0].data_ptr(), out['dstn'][1].data_ptr()
        if backward:
            mn = torch.randint(0, 256, (P, C // 8), generator=g, dtype=torch.uint8).cuda()
            keep.append(mn)
            d.mask_next = mn.data_ptr()
        else:
            bn = torch.randn(C, generator=g).cuda() * 0.3
            keep.append(bn)
            out['sign_next'] = torch.full((P, C // 8), 0xAA, dtype=torch.uint8, device='cuda')
            d.bias_next, d.sign_next, d.relu_next = bn.data_ptr(), out['sign_next'].data_ptr(), 1
    return d, out, keep


def _bits_of(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


@gpu
@pytest.mark.parametrize('B,H,W', GEOMETRIES)
@pytest.mark.parametrize('mode', MODES)
def test_slab_staging_is_bit_identical_to_per_tap_staging(mode, B, H, W):
    from robustart_amd import _lib
    lib = _lib.load()
    d, out, keep = _case(_lib, mode, B, H, W)
    expect = {'dst'} | ({'dstn'} if mode.endswith('next') else set()) | (set() if mode.startswith('bwd') else {'sign_mid', 'sign_out'}) \
        | ({'sign_next'} if mode in ('fwd_next', 'xs_next') else set())
    assert set(out) == expect
    old = lib.rart_conv3x3_tail_pair_get_staging()
    got = {}
    try:
        for staging in (0, 1):
            _lib.check(lib.rart_conv3x3_tail_pair_set_staging(staging))
            for name, t in out.items():
                t.fill_(float('nan') if t.dtype == torch.bfloat16 else 0xAA)
            _lib.check(lib.rart_conv3x3_tail_pair(ctypes.byref(d), _lib.stream_ptr()))
            torch.cuda.synchronize()
            got[staging] = {name: t.clone() for name, t in out.items()}
    finally:
        lib.rart_conv3x3_tail_pair_set_staging(0)
        lib.rart_conv3x3_tail_pair_set_staging(old)
    for name in sorted(out):
        for staging in (0, 1):
            if out[name].dtype == torch.bfloat16:
                assert torch.isfinite(got[staging][name].float()).all(), (name, staging)
        assert torch.equal(_bits_of(got[1][name]), _bits_of(got[0][name])), name
    assert got[0]['dst'].float().abs().max().item() > 0.1          # a launch that wrote zeros everywhere would pass the lines above


@gpu
def test_engine_forward_backward_is_bit_identical_under_both_stagings():
    """ResNet50Engine(precision='fp32x').forward_backward on 3 x 3 x 96 x 128 (layer1 at 24 x 32: six tail launches on the slab path, tiles
    that span images) with staging 0 and 1: torch.equal logits and input gradient."""
    from robustart_amd import _lib
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    lib = _lib.load()
    torch.manual_seed(0)
    m = randomize_bn_stats(get_model({'type': 'resnet50_official'}), 0).eval().cuda()
    for p in m.parameters():
        p.requires_grad_(False)
    eng = ResNet50Engine(m, 'cuda', precision='fp32x')
    assert eng.fused_tail_pair
    g = torch.Generator().manual_seed(43)
    x = torch.rand(3, 3, 96, 128, generator=g).cuda()
    y = torch.randint(0, 1000, (3,), generator=g).cuda()
    old = lib.rart_conv3x3_tail_pair_get_staging()
    res = {}
    try:
        for staging in (0, 1):
            _lib.check(lib.rart_conv3x3_tail_pair_set_staging(staging))
            logits, _, grad, _ = eng.forward_backward(x, MEAN, STD, y, 0)
            res[staging] = (logits.clone(), grad.clone())
    finally:
        lib.rart_conv3x3_tail_pair_set_staging(0)
        lib.rart_conv3x3_tail_pair_set_staging(old)
    assert torch.isfinite(res[1][0]).all() and torch.isfinite(res[1][1]).all()
    assert torch.equal(res[1][0], res[0][0])
    assert torch.equal(res[1][1], res[0][1])
