"""Reference-precision ResNet-50: the projection shortcut of a layer's first block folded into the launch it is added in.

  * rart_gemm_pair2_bf16: a conv-mode pair launch with a SECOND A source: yc = relu(W3 . yb + Wds . x_strided + (b3 + bds)) is one accumulation, the
    shortcut's K steps follow conv3's, the table's rows are [W3 | Wds];
  * rart_conv3x3_tail_pair with the shortcut's input as extra K steps of its 1x1 phase (layer1's first block);
  * the engine switch `fused_shortcut_pair` against the chain with the shortcut on its own launch.

Bounds are the project's own for these kernels: 2.5e-5 of the output scale for the pair conv kernel against fp64 of the same hi / lo
operands (test_pair_conv_kernel_vs_fp64), 2e-5 / 1e-5 for the tail kernel and its neighbour reduction (test_conv_tail_pair_kernel_vs_fp64),
2e-5 of the logit scale between two summation orders of the engine (test_x3_fused_tail_matches_the_two_launch_path) and 1e-4 against the
fp32 module."""
import ctypes
import functools

import pytest
import torch

gpu = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _split(t):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


def _f64(p):
    return p[0].double() + p[1].double()


def _bits(t, n):
    """1-bit tensor [P][n / 8] -> [P][n] of 0 / 1"""
    return torch.stack([(t >> j) & 1 for j in range(8)], -1).reshape(t.shape[0], n)


def _cat_table(w1, w2):
    """-> (pair of w1, pair of w2, the [hi | lo | hi] table of the rows [w1 | w2])"""
    p1, p2 = _split(w1), _split(w2)
    return p1, p2, torch.cat([p1[0], p2[0], p1[1], p2[1], p1[0], p2[0]], 1).contiguous()


@functools.lru_cache(maxsize=None)
def _two_source_case(backward):
    """Inputs and the fp64 result of one two-source launch, computed once for every tile of the parametrisation.
    forward : 3 x 10 x 9 rows (270: a full 256-row tile and a ragged one), source 1 = 64 channels at the grid's size, source 2 = 128
              channels of a 20 x 18 image read at stride 2, N = 152 (a ragged column tile), bias + ReLU + sign bits;
    backward: layer1.0's shape -- K1 = 64, k2 = 256 at stride 1, N = 64, 1-bit mask, no bias, no ReLU."""
    g = torch.Generator().manual_seed(17 + backward)
    B, Gh, Gw = 3, 10, 9
    if backward:
        C1, C2, N, s2 = 64, 256, 64, 1
    else:
        C1, C2, N, s2 = 64, 128, 152, 2
    a1 = _split(torch.randn(B, Gh, Gw, C1, generator=g).cuda())
    a2 = _split(torch.randn(B, Gh * s2, Gw * s2, C2, generator=g).cuda())
    w1 = (torch.randn(N, C1, generator=g) * 0.08).cuda()
    w2 = (torch.randn(N, C2, generator=g) * 0.08).cuda()
    p1, p2, tab = _cat_table(w1, w2)
    bias = torch.randn(N, generator=g).cuda()
    mask = torch.randint(0, 256, (B * Gh * Gw, N // 8), generator=g, dtype=torch.uint8).cuda()
    want = _f64(a1).reshape(-1, C1) @ _f64(p1).t() + _f64(a2)[:, ::s2, ::s2].reshape(-1, C2) @ _f64(p2).t()
    if backward:
        want = want * _bits(mask, N).double()
    else:
        want = torch.relu(want + bias.double())
    return dict(B=B, Gh=Gh, Gw=Gw, C1=C1, C2=C2, N=N, s2=s2, a1=a1, a2=a2, tab=tab, bias=bias, mask=mask, want=want)


def _two_source_desc(_lib, c, backward, out, sign, tile_n, tile_m):
    d2 = _lib.GemmPair2Desc()
    d = d2.one
    K = c['C1'] + c['C2']
    d.a_hi, d.a_lo, d.w_hi, d.w_lo = c['a1'][0].data_ptr(), c['a1'][1].data_ptr(), c['tab'].data_ptr(), c['tab'].data_ptr() + 2 * K
    d.dst_hi, d.dst_lo = out[0].data_ptr(), out[1].data_ptr()
    d.N, d.lda, d.ldw, d.ldc, d.w_rows, d.tile_n, d.tile_m = c['N'], c['C1'], 3 * K, c['N'], c['N'], tile_n, tile_m
    d.conv, d.batch, d.grid_h, d.grid_w, d.src_h, d.src_w, d.sy, d.sx, d.k_per_tap, d.n_taps = 1, c['B'], c['Gh'], c['Gw'], c['Gh'], c['Gw'], 1, 1, c['C1'], 1
    d.dst_h, d.dst_w, d.dst_sy, d.dst_sx = c['Gh'], c['Gw'], 1, 1
    d2.a2_hi, d2.a2_lo = c['a2'][0].data_ptr(), c['a2'][1].data_ptr()
    d2.lda2, d2.k2, d2.src2_h, d2.src2_w, d2.sy2, d2.sx2 = c['C2'], c['C2'], c['Gh'] * c['s2'], c['Gw'] * c['s2'], c['s2'], c['s2']
    if backward:
        d.mask_bits = c['mask'].data_ptr()
    else:
        d.bias, d.flags, d.sign_out = c['bias'].data_ptr(), 1, sign.data_ptr()
    return d2


def _run_two_source(backward, tile_n, tile_m):
    from robustart_amd import _lib
    lib = _lib.load()
    c = _two_source_case(backward)
    M, N = c['B'] * c['Gh'] * c['Gw'], c['N']
    out = torch.full((2, M, N), float('nan'), dtype=torch.bfloat16, device='cuda')
    sign = torch.zeros(M, N // 8, dtype=torch.uint8, device='cuda')
    d = _two_source_desc(_lib, c, backward, out, sign, tile_n, tile_m)
    _lib.check(lib.rart_gemm_pair2_bf16(ctypes.byref(d), _lib.stream_ptr()))
    torch.cuda.synchronize()
    got, want = _f64(out), c['want']
    assert torch.isfinite(got).all()
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print('two-source pair conv (%s) tile %d x %d: scale %.3f, max |err| %.3g (%.2g of scale)'
          % ('backward shape' if backward else 'forward shape', tile_m, tile_n, scale, err, err / scale))
    assert err <= 2.5e-5 * scale
    return lib, _lib, d, out, sign


@gpu
@pytest.mark.parametrize('tile_n,tile_m', [(0, 0), (64, 256), (64, 128), (128, 128),        # the two-stage kernel
                                           (128, 256), (256, 256), (256, 224)])             # the ping-pong kernel and its 224-row form
def test_two_source_pair_conv_vs_fp64(tile_n, tile_m):
    """conv3 + stride-2 projection shortcut as one launch against fp64 of the same hi / lo operands, under the default schedule and under
    schedule 0, every tile form; the sign bytes are those of the stored hi plane; malformed second sources are argument errors."""
    lib, _lib, d, out, sign = _run_two_source(False, tile_n, tile_m)
    assert torch.equal(_bits(sign, out.shape[2]).bool(), out[0].float() > 0)
    first = out.view(torch.int16).clone()
    old = lib.rart_gemm_pair_get_schedule()
    try:       # schedule 0 sends every tile to the two-stage loop: the same products in the same order
        _lib.check(lib.rart_gemm_pair_set_schedule(0))
        out.fill_(float('nan'))
        _lib.check(lib.rart_gemm_pair2_bf16(ctypes.byref(d), _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), first)
    finally:
        lib.rart_gemm_pair_set_schedule(old)
    assert lib.rart_gemm_pair_max_sources() == 2
    for owner, field, bad in ((d, 'k2', 48), (d, 'lda2', 12), (d.one, 'n_batched', 2), (d, 'a2_lo', None), (d, 'sy2', 3)):
        keep = getattr(owner, field)
        setattr(owner, field, bad)
        assert lib.rart_gemm_pair2_bf16(ctypes.byref(d), _lib.stream_ptr()) != 0, field
        setattr(owner, field, keep)


@gpu
@pytest.mark.parametrize('tile_n,tile_m', [(0, 0), (64, 256), (64, 128)])
def test_two_source_pair_conv_backward_shape_vs_fp64(tile_n, tile_m):
    """dx = mask(W1^T . dza + Wds^T . dz) of layer1's first block: K1 = 64, k2 = 256 at stride 1, N = 64, 1-bit mask, no ReLU."""
    _run_two_source(True, tile_n, tile_m)


@gpu
@pytest.mark.parametrize('conv,M,K,N,tile_n', [
    (None, 1000, 96, 384, 256),
    ((3, 12, 10, 32), 360, 288, 128, 128),
    ((4, 33, 32, 128), 4224, 1152, 512, 256),
])
def test_single_source_launches_are_untouched(conv, M, K, N, tile_n):
    """rart_gemm_pair_bf16 under the default schedule, and rart_gemm_pair2_bf16 on the same launch with a null second source -- its other
    fields zero, then set to values a two-source launch would refuse -- give the bits of the schedule-0 path: the second source's fields
    are read only behind a2_hi."""
    from robustart_amd import _lib
    from test_engine_x3_gpu import _pair_schedule_case
    lib = _lib.load()
    d, out, sign, keep = _pair_schedule_case(lib, _lib, conv, M, K, N, tile_n, False, seed=11)
    d2 = _lib.GemmPair2Desc()
    ctypes.memmove(ctypes.byref(d2.one), ctypes.byref(d), ctypes.sizeof(d))
    assert not d2.a2_hi and not d2.a2_lo and (d2.lda2, d2.k2, d2.src2_h, d2.src2_w, d2.sy2, d2.sx2) == (0,) * 6
    old = lib.rart_gemm_pair_get_schedule()
    try:
        _lib.check(lib.rart_gemm_pair_set_schedule(0))
        _lib.check(lib.rart_gemm_pair_bf16(ctypes.byref(d), _lib.stream_ptr()))
        torch.cuda.synchronize()
        want, want_sign = out.view(torch.int16).clone(), sign.clone()
        assert torch.isfinite(out.float()).all()
        _lib.check(lib.rart_gemm_pair_set_schedule(1))
        for form in (0, 1, 2):
            if form == 2:
                d2.lda2, d2.k2, d2.src2_h, d2.src2_w, d2.sy2, d2.sx2 = 12, 48, -1, 7, 0, 3
            out.fill_(float('nan'))
            sign.zero_()
            _lib.check(lib.rart_gemm_pair2_bf16(ctypes.byref(d2), _lib.stream_ptr()) if form else
                       lib.rart_gemm_pair_bf16(ctypes.byref(d), _lib.stream_ptr()))
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int16), want) and torch.equal(sign, want_sign)
    finally:
        lib.rart_gemm_pair_set_schedule(old)


@gpu
@pytest.mark.parametrize('nxt', [False, True])
def test_conv_tail_pair_with_the_shortcut_source_vs_fp64(nxt):
    """rart_conv3x3_tail_pair, forward, C = 64, with the block's 1x1 projection shortcut as extra K steps of the 1x1 phase:
    out = relu(W3 . relu(W2 * a + b2) + Wds . x + (b3 + bds)) against fp64 of the same pair operands, the intermediate rounded to a pair
    where the kernel rounds it.  2 x 9 x 7 = 126 positions: a ragged 128-position tile.  nxt: the next block's reduction in the launch."""
    from robustart_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(64 + nxt)
    B, H, W, C = 2, 9, 7, 64
    N, P = 4 * C, B * H * W
    a = _split(torch.randn(B, H, W, C, generator=g).cuda())
    x = _split(torch.randn(B, H, W, C, generator=g).cuda())
    w2 = (torch.randn(C, 3, 3, C, generator=g) * (2.0 / (9 * C)) ** 0.5).cuda()             # [n][r][s][c]
    w3 = (torch.randn(N, C, generator=g) * (1.0 / C) ** 0.5).cuda()
    wd = (torch.randn(N, C, generator=g) * (1.0 / C) ** 0.5).cuda()
    b2, bsum = torch.randn(C, generator=g).cuda() * 0.3, torch.randn(N, generator=g).cuda() * 0.3
    w2p, w3p, wdp = _split(w2.reshape(C, 9 * C)), _split(w3), _split(wd)
    tab = torch.cat([w2p[0], w2p[1], w2p[0]], 1).contiguous()
    frag = lambda p: torch.stack([p[pl].reshape(N // 32, 32, C // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)    # noqa: E731
                                  for pl in range(2)]).contiguous()
    tail, tx = frag(w3p), frag(wdp)
    dst = torch.full((2, B, H, W, N), float('nan'), dtype=torch.bfloat16, device='cuda')
    sm = torch.full((P, C // 8), 0xAA, dtype=torch.uint8, device='cuda')
    so = torch.full((P, N // 8), 0xAA, dtype=torch.uint8, device='cuda')
    d = _lib.ConvTailDesc()
    d.a_hi, d.a_lo, d.w_hi, d.w_lo = a[0].data_ptr(), a[1].data_ptr(), tab.data_ptr(), tab.data_ptr() + 2 * 9 * C
    d.t_hi, d.t_lo, d.dst_hi, d.dst_lo = tail[0].data_ptr(), tail[1].data_ptr(), dst[0].data_ptr(), dst[1].data_ptr()
    d.x_hi, d.x_lo, d.tx_hi, d.tx_lo = x[0].data_ptr(), x[1].data_ptr(), tx[0].data_ptr(), tx[1].data_ptr()
    d.batch, d.h, d.w, d.c_mid, d.ldw = B, H, W, C, 3 * 9 * C
    for i in range(9):
        d.tap_dy[i], d.tap_dx[i] = i // 3 - 1, i % 3 - 1
    d.bias_mid, d.bias_out, d.sign_mid, d.sign_out = b2.data_ptr(), bsum.data_ptr(), sm.data_ptr(), so.data_ptr()
    d.relu_mid = d.relu_out = 1
    if nxt:
        wn = (torch.randn(C, N, generator=g) * (1.0 / N) ** 0.5).cuda()
        wnp = _split(wn)
        ntab = torch.stack([wnp[pl].reshape(C // 32, 32, N // 64, 4, 2, 8).permute(2, 0, 3, 4, 1, 5).contiguous().view(-1)
                            for pl in range(2)]).contiguous()
        dn = torch.full((2, P, C), float('nan'), dtype=torch.bfloat16, device='cuda')
        bn = torch.randn(C, generator=g).cuda() * 0.3
        sn = torch.full((P, C // 8), 0xAA, dtype=torch.uint8, device='cuda')
        d.n_hi, d.n_lo, d.dstn_hi, d.dstn_lo = ntab[0].data_ptr(), ntab[1].data_ptr(), dn[0].data_ptr(), dn[1].data_ptr()
        d.bias_next, d.sign_next, d.relu_next = bn.data_ptr(), sn.data_ptr(), 1
    _lib.check(lib.rart_conv3x3_tail_pair(ctypes.byref(d), _lib.stream_ptr()))
    torch.cuda.synchronize()
    a64 = _f64(a).permute(0, 3, 1, 2)
    w64 = _f64(w2p).reshape(C, 3, 3, C).permute(0, 3, 1, 2)
    mid = (torch.nn.functional.conv2d(a64, w64, padding=1).permute(0, 2, 3, 1).reshape(P, C) + b2.double()).clamp_min(0)
    want = (_f64(_split(mid.float())) @ _f64(w3p).t() + _f64(x).reshape(P, C) @ _f64(wdp).t() + bsum.double()).clamp_min(0)
    got = _f64(dst).reshape(P, N)
    assert torch.isfinite(got).all()
    err = (got - want).abs().max().item() / want.abs().max().item()
    print('conv tail pair with the shortcut source, nxt=%s: max err %.2e of scale' % (nxt, err))
    assert err <= 2e-5
    assert torch.equal(_bits(so, N), (dst[0].reshape(P, N) > 0).to(torch.uint8))
    clear = mid.abs() > 1e-3
    assert torch.equal(_bits(sm, C)[clear], (mid > 0).to(torch.uint8)[clear])
    if nxt:
        nref = (got @ _f64(wnp).t() + bn.double()).clamp_min(0)        # the reduction multiplies the pair the kernel WROTE
        ngot = _f64(dn)
        assert torch.isfinite(ngot).all()
        nerr = (ngot - nref).abs().max().item() / nref.abs().max().item()
        print('   neighbour reduction: max err %.2e of scale' % nerr)
        assert nerr <= 1e-5
        assert torch.equal(_bits(sn, C), (dn[0] > 0).to(torch.uint8))
    # the shortcut source takes the place of the skip pair, and needs all four planes
    d.res_hi, d.res_lo = dst[0].data_ptr(), dst[1].data_ptr()
    assert lib.rart_conv3x3_tail_pair(ctypes.byref(d), _lib.stream_ptr()) != 0
    d.res_hi = d.res_lo = None
    d.tx_lo = None
    assert lib.rart_conv3x3_tail_pair(ctypes.byref(d), _lib.stream_ptr()) != 0


@gpu
def test_x3_fused_shortcut_matches_the_separate_launch():
    """The reference-precision engine with every projection shortcut folded into the launch it is added in against the same engine with the
    shortcuts on their own launches: one rounding fewer and another fp32 summation order, nothing else.  A fresh engine allocates no
    shortcut buffer in its forward: the pass is gone, not hidden."""
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    torch.manual_seed(0)
    m = randomize_bn_stats(get_model({'type': 'resnet50_official'}), 0).eval().cuda()
    for p in m.parameters():
        p.requires_grad_(False)
    eng = ResNet50Engine(m, 'cuda', precision='fp32x')
    g = torch.Generator().manual_seed(41)
    x = torch.rand(3, 3, 96, 128, generator=g).cuda()
    y = torch.randint(0, 1000, (3,), generator=g).cuda()
    assert eng.fused_shortcut_pair
    assert all(getattr(b[3], 'w_cat', None) is not None for b in eng.blocks if b[3] is not None)
    assert getattr(eng.blocks[0][3], 'tail_x', None) is not None and getattr(eng.blocks[0][3], 'w_cat_bwd', None) is not None
    lf = eng.logits(x, MEAN, STD).clone()
    assert not [k for k in eng._buf if k.endswith('_ds')], 'the forward still writes a shortcut tensor'
    la, _, ga, _ = eng.forward_backward(x, MEAN, STD, y, 0)
    la, ga = la.clone(), ga.clone()
    assert torch.equal(la, lf)
    assert not [k for k in eng._buf if k.endswith('_ds')]
    eng.fused_shortcut_pair = False
    try:
        lb, _, gb, _ = eng.forward_backward(x, MEAN, STD, y, 0)
    finally:
        eng.fused_shortcut_pair = True
    assert len([k for k in eng._buf if k.endswith('_ds')]) == 4
    le = (la - lb).abs().max().item() / lb.abs().max().item()
    a, b = ga.double().flatten(1), gb.double().flatten(1)
    rel = ((a - b).norm(dim=1) / b.norm(dim=1)).max().item()
    cos = ((a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).min().item()
    mean = torch.tensor(MEAN, device='cuda').view(1, 3, 1, 1)
    std = torch.tensor(STD, device='cuda').view(1, 3, 1, 1)
    ref = m((x - mean) / std)
    lt = (la - ref).abs().max().item() / ref.abs().max().item()
    print('x3 fused shortcut vs its own launch: logits %.2e of scale (bit-equal: %s), gradient rel L2 %.2e, cos %.6f; vs fp32 torch %.2e'
          % (le, torch.equal(la, lb), rel, cos, lt))
    assert le <= 2e-5
    assert rel <= 0.15 and cos >= 0.98          # ReLU decisions of near-zero pre-activations may flip
    assert lt <= 1e-4


@pytest.mark.parametrize('stride', [2, 1])
def test_fold_shortcut_tables_cpu(stride):
    """(no GPU) the concatenated table and the bias sum of a small random Bottleneck with a projection equal cat([W3, Wds], K) and
    b3 + bds of the folded fp32 weights after the hi / lo split; a stride-1 projection also gets the transposed pair [W1^T | Wds^T]."""
    from robustart_amd.model.engine import _Conv, fold_shortcut_tables
    from robustart_amd.model.resnet_torch import Bottleneck
    torch.manual_seed(5 + stride)
    cin, planes = 64, 32
    ds = torch.nn.Sequential(torch.nn.Conv2d(cin, 4 * planes, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(4 * planes))
    blk = Bottleneck(cin, planes, stride, ds).eval()
    for mod in blk.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.5)
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.3)
    ca, cc, cd = (_Conv(blk.conv1, blk.bn1, 'cpu', split=True), _Conv(blk.conv3, blk.bn3, 'cpu', split=True),
                  _Conv(blk.downsample[0], blk.downsample[1], 'cpu', split=True))
    assert fold_shortcut_tables(ca, cc, cd)

    def table(w):
        hi = w.to(torch.bfloat16)
        lo = (w - hi.float()).to(torch.bfloat16)
        return torch.cat([hi, lo, hi], 1)
    w3, wd = cc.w_folded.reshape(4 * planes, planes), cd.w_folded.reshape(4 * planes, cin)
    assert cd.w_cat.shape == (4 * planes, 3 * (planes + cin))
    assert torch.equal(cd.w_cat, table(torch.cat([w3, wd], 1)))
    assert torch.equal(cd.bias_cat, cc.b_folded + cd.b_folded)
    if stride == 1:
        w1 = ca.w_folded.reshape(planes, cin)
        assert torch.equal(cd.w_cat_bwd, table(torch.cat([w1.t(), wd.t()], 1)))
    else:
        assert getattr(cd, 'w_cat_bwd', None) is None
