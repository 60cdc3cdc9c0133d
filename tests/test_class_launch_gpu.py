"""Reference-precision ResNet-50: the input-parity classes of a stride-2 backward-to-input in ONE launch.

  * rart_gemm_pair_classes_bf16: up to four classes of a conv-mode pair launch in one grid (blockIdx.y = class), each with its own taps, its
    slice of the weight rows, its K length and its destination parity -- bit for bit what the classes' own launches write;
  * class 0 with a second A source: dx = mask(W1^T . dza + Wds^T . dz) on the parity (0, 0) of a stride-2 first block, one accumulation
    where the two-launch form rounds dx to a pair in between;
  * the engine switches `pair_class_launch` / `class_shortcut_channels` against the chain with one launch per class.

Geometry of the kernel tests: B = 2, dx 6 x 10, dz 3 x 5 -- 30 rows per class: a ragged tile, M no multiple of 32."""
import ctypes
import functools

import pytest
import torch

gpu = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
B, GH, GW = 2, 3, 5          # the row grid of a class = dz's size; dx is 2 GH x 2 GW
PARITIES = ((0, 0), (0, 1), (1, 0), (1, 1))


def _split(t):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


def _f64(p):
    return p[0].double() + p[1].double()


def _bits(t, n):
    """1-bit tensor [P][n / 8] -> [P][n] of 0 / 1"""
    return torch.stack([(t >> j) & 1 for j in range(8)], -1).reshape(t.shape[0], n)


def _classes(kind):
    """-> [(parity, taps)] of the backward-to-input of a 3x3 / 2 pad-1 convolution ('3x3': dz read at stride 1, 1 / 2 / 2 / 4 taps) or of a
    1x1 read at the four parities of a full-size gradient ('1x1': stride 2, the tap is the parity)"""
    if kind == '1x1':
        return [(p, [p]) for p in PARITIES]
    from robustart_amd.model.engine_base import conv_tap_classes
    return [(parity, taps) for parity, taps, _ in conv_tap_classes(3, 3, 2, 1)[2]]


@functools.lru_cache(maxsize=None)
def _case(kind, C, N, k2=0):
    """Operands of one class launch, made once: source pair, the class-ordered [hi | lo] table (class 0's slice followed by the second
    source's k2 columns), a 1-bit mask over dx, the second source."""
    g = torch.Generator().manual_seed(1000 + C + N + (kind == '1x1'))
    cls = _classes(kind)
    sh, sw = (GH, GW) if kind == '3x3' else (2 * GH, 2 * GW)
    src = _split(torch.randn(B, sh, sw, C, generator=g).cuda())
    ks = [C * len(taps) + (k2 if i == 0 else 0) for i, (_, taps) in enumerate(cls)]
    offs = [sum(ks[:i]) for i in range(len(ks))]
    w = _split((torch.randn(N, sum(ks), generator=g) * 0.05).cuda())
    tab = torch.cat([w[0], w[1]], 1).contiguous()                         # rows [hi | lo]: ldw = 2 K, w_lo = w_hi + K
    mask = torch.randint(0, 256, (B * 2 * GH * 2 * GW, N // 8), generator=g, dtype=torch.uint8).cuda()
    src2 = _split(torch.randn(B, GH, GW, k2, generator=g).cuda()) if k2 else None
    return dict(kind=kind, C=C, N=N, k2=k2, cls=cls, src=src, src_hw=(sh, sw), ks=ks, offs=offs, w=w, tab=tab, mask=mask, src2=src2,
                stride=1 if kind == '3x3' else 2)


def _fill_one(d, c, out, taps, masked, tile):
    """the fields the classes of case c share, taps = [(dy, dx)] in the slots"""
    K = sum(c['ks'])
    d.a_hi, d.a_lo = c['src'][0].data_ptr(), c['src'][1].data_ptr()
    d.w_hi, d.w_lo = c['tab'].data_ptr(), c['tab'].data_ptr() + 2 * K
    d.dst_hi, d.dst_lo = out[0].data_ptr(), out[1].data_ptr()
    d.N, d.lda, d.ldw, d.ldc, d.w_rows = c['N'], c['C'], 2 * K, c['N'], c['N']
    d.tile_m, d.tile_n = tile
    d.conv, d.batch, d.grid_h, d.grid_w = 1, B, GH, GW
    d.src_h, d.src_w, d.sy, d.sx, d.k_per_tap, d.n_taps = c['src_hw'][0], c['src_hw'][1], c['stride'], c['stride'], c['C'], len(taps)
    for i, (dy, dx) in enumerate(taps):
        d.tap_dy[i], d.tap_dx[i] = dy, dx
    d.dst_h, d.dst_w, d.dst_sy, d.dst_sx = 2 * GH, 2 * GW, 2, 2
    if masked:
        d.mask_bits = c['mask'].data_ptr()


def _class_desc(_lib, c, out, masked, tile, with_src2=False):
    d = _lib.GemmPairClsDesc()
    _fill_one(d.two.one, c, out, [t for _, taps in c['cls'] for t in taps], masked, tile)
    d.n_classes = len(c['cls'])
    at = 0
    for i, (parity, taps) in enumerate(c['cls']):
        k = d.cls[i]
        k.tap_begin, k.n_taps, k.k_off, k.dst_oy, k.dst_ox, k.src2 = at, len(taps), c['offs'][i], parity[0], parity[1], int(with_src2 and i == 0)
        at += len(taps)
    if with_src2:
        s2 = c['src2']
        d.two.a2_hi, d.two.a2_lo = s2[0].data_ptr(), s2[1].data_ptr()
        d.two.lda2, d.two.k2, d.two.src2_h, d.two.src2_w, d.two.sy2, d.two.sx2 = c['k2'], c['k2'], GH, GW, 1, 1
    return d


def _separate(lib, _lib, c, out, masked):
    """every class as a launch of its own on rart_gemm_pair_bf16 (its slice of the table through the plane pointers), automatic tiles"""
    for i, (parity, taps) in enumerate(c['cls']):
        d = _lib.GemmPairDesc()
        _fill_one(d, c, out, taps, masked, (0, 0))
        d.w_hi, d.w_lo = d.w_hi + 2 * c['offs'][i], d.w_lo + 2 * c['offs'][i]
        d.dst_oy, d.dst_ox = parity
        _lib.check(lib.rart_gemm_pair_bf16(ctypes.byref(d), _lib.stream_ptr()))


@gpu
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('kind,C,N,tile', [
    ('3x3', 64, 32, (0, 0)), ('1x1', 64, 32, (0, 0)),                  # the two-stage kernel (automatic tiles: 128 x 64 at 30 rows)
    ('3x3', 256, 256, (0, 0)), ('1x1', 256, 256, (0, 0)),
    ('3x3', 256, 256, (256, 256)), ('1x1', 256, 256, (256, 256)),      # the ping-pong kernel
    ('3x3', 256, 256, (224, 256)),                                     # ... and its 224-row form
])
def test_class_launch_equals_the_separate_launches(kind, C, N, tile, masked):
    """One class launch writes the bits of the four per-class launches: the products and their order per element are the same."""
    from robustart_amd import _lib
    lib = _lib.load()
    assert lib.rart_gemm_pair_max_classes() == 4
    c = _case(kind, C, N)
    shape = (2, B, 2 * GH, 2 * GW, N)
    want = torch.full(shape, float('nan'), dtype=torch.bfloat16, device='cuda')
    _separate(lib, _lib, c, want, masked)
    got = torch.full(shape, float('nan'), dtype=torch.bfloat16, device='cuda')
    d = _class_desc(_lib, c, got, masked, tile)
    _lib.check(lib.rart_gemm_pair_classes_bf16(ctypes.byref(d), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all() and torch.isfinite(got.float()).all()        # every pixel of dx belongs to exactly one class
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    if masked:
        keep = _bits(c['mask'], N).bool().reshape(shape[1:])
        assert (got[0][~keep] == 0).all() and (got[1][~keep] == 0).all()


@gpu
def test_class0_second_source_vs_fp64():
    """dx = mask(W1^T . dza + Wds^T . dz) of a stride-2 first block at layer2's widths (K1 = 128 per class, k2 = 512 on class (0, 0),
    N = 256) against fp64 of the same pair operands, next to the two-launch form it replaces: conv1^T over all of dx, then the
    shortcut^T launch that reads dx's parity (0, 0) back as its residual and rounds the sum to a pair a second time.

    The bound is the two-launch form's own error on the same inputs, no margin.  The figure is the relative L2 error over the class
    (0, 0) (the only elements that differ): both forms share the fp32 accumulation and the dropped lo.lo products, the fused one drops one
    pair rounding (2^-17 relative per element), so its squared error is smaller by that rounding's variance in expectation, while the
    maximum over 7680 elements is decided by single elements where either form may land nearer.  The other three classes are bit-equal.
    Measured on MI355X: relative L2 3.636e-06 fused against 3.802e-06 as two launches (maximum error 4.65e-06 of scale in both)."""
    from robustart_amd import _lib
    lib = _lib.load()
    C, N, k2 = 128, 256, 512
    c = _case('1x1', C, N, k2)
    shape = (2, B, 2 * GH, 2 * GW, N)
    # ---- the two-launch form: W1^T . dza over the whole of dx (one tap, stride 1), then + Wds^T . dz on the parity (0, 0)
    two = torch.full(shape, float('nan'), dtype=torch.bfloat16, device='cuda')
    K = sum(c['ks'])
    d = _lib.GemmPairDesc()
    _fill_one(d, c, two, [(0, 0)], True, (0, 0))
    d.grid_h, d.grid_w, d.sy, d.sx, d.dst_sy, d.dst_sx = 2 * GH, 2 * GW, 1, 1, 1, 1
    _lib.check(lib.rart_gemm_pair_bf16(ctypes.byref(d), _lib.stream_ptr()))
    s2 = c['src2']
    d = _lib.GemmPairDesc()
    _fill_one(d, c, two, [(0, 0)], True, (0, 0))
    d.a_hi, d.a_lo, d.lda, d.k_per_tap = s2[0].data_ptr(), s2[1].data_ptr(), k2, k2
    d.src_h, d.src_w, d.sy, d.sx = GH, GW, 1, 1
    d.w_hi, d.w_lo = d.w_hi + 2 * C, d.w_lo + 2 * C                      # class 0's slice is [W1^T | Wds^T]
    d.res_hi, d.res_lo = two[0].data_ptr(), two[1].data_ptr()
    _lib.check(lib.rart_gemm_pair_bf16(ctypes.byref(d), _lib.stream_ptr()))
    # ---- the class launch
    got = torch.full(shape, float('nan'), dtype=torch.bfloat16, device='cuda')
    d = _class_desc(_lib, c, got, True, (0, 0), with_src2=True)
    _lib.check(lib.rart_gemm_pair_classes_bf16(ctypes.byref(d), _lib.stream_ptr()))
    torch.cuda.synchronize()
    w64 = _f64(c['w'])
    wd = w64[:, C:C + k2]
    keep = _bits(c['mask'], N).double().reshape(shape[1:])
    src = _f64(c['src'])
    want = torch.empty(shape[1:], dtype=torch.float64, device='cuda')
    for i, (ph, pw) in enumerate(PARITIES):
        wi = w64[:, c['offs'][i]:c['offs'][i] + C]
        want[:, ph::2, pw::2] = src[:, ph::2, pw::2] @ wi.t()
    want[:, 0::2, 0::2] += _f64(s2) @ wd.t()
    want *= keep
    assert torch.isfinite(got.float()).all() and torch.isfinite(two.float()).all()
    # the two forms are compared on the class (0, 0): there both multiply dza by class 0's slice W1^T (the case draws the other three
    # slices independently, and the two-launch form runs W1^T over every parity)
    g0, t0, r0 = _f64(got)[:, 0::2, 0::2], _f64(two)[:, 0::2, 0::2], want[:, 0::2, 0::2]
    err_fused = ((g0 - r0).norm() / r0.norm()).item()
    err_two = ((t0 - r0).norm() / r0.norm()).item()
    print('class 0 with the second source vs fp64: relative L2 fused %.4g, two launches %.4g; max |err| of scale fused %.3g, two launches %.3g'
          % (err_fused, err_two, ((g0 - r0).abs().max() / r0.abs().max()).item(), ((t0 - r0).abs().max() / r0.abs().max()).item()))
    assert err_fused <= err_two
    # the classes without the second source, against their own fp64 result: the pair conv kernel's bound (test_pair_conv_kernel_vs_fp64)
    scale = want.abs().max().item()
    assert (_f64(got) - want).abs().max().item() <= 2.5e-5 * scale


def test_class_launch_argument_checks():
    """(no GPU) malformed class tables are argument errors before any launch: more than four classes, taps past the sixteen slots or past
    the filled ones, a second source on a class other than 0 or without its planes, a slice outside the weight rows, a destination
    origin outside the image, an interleaved weight table."""
    from robustart_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint16 * 16)()
    p = ctypes.addressof(buf)

    def fresh():
        d = _lib.GemmPairClsDesc()
        o = d.two.one
        o.a_hi = o.a_lo = o.w_hi = o.w_lo = o.dst_hi = o.dst_lo = p
        o.N, o.lda, o.ldw, o.ldc, o.w_rows = 32, 64, 9 * 64 * 2, 32, 32
        o.conv, o.batch, o.grid_h, o.grid_w, o.src_h, o.src_w, o.sy, o.sx, o.k_per_tap, o.n_taps = 1, 2, 3, 5, 3, 5, 1, 1, 64, 9
        o.dst_h, o.dst_w, o.dst_sy, o.dst_sx = 6, 10, 2, 2
        d.n_classes = 4
        at = 0
        for i, (n, (oy, ox)) in enumerate(zip((1, 2, 2, 4), PARITIES)):
            k = d.cls[i]
            k.tap_begin, k.n_taps, k.k_off, k.dst_oy, k.dst_ox = at, n, at * 64, oy, ox
            at += n
        return d

    def refused(d, why):
        """the call fails, and for the reason meant: `why` is part of the message"""
        assert lib.rart_gemm_pair_classes_bf16(ctypes.byref(d) if d is not None else None, None) != 0
        msg = lib.rart_last_error_string().decode()
        assert why in msg, msg

    refused(None, 'null descriptor')
    d = fresh(); d.n_classes = 5
    refused(d, '1..4 classes')
    d = fresh(); d.n_classes = 0
    refused(d, '1..4 classes')
    d = fresh(); d.cls[3].tap_begin, d.cls[3].n_taps = 13, 4              # past the sixteen slots
    refused(d, 'tap slots')
    d = fresh(); d.cls[3].n_taps = 5                                       # past the filled slots
    refused(d, 'tap slots')
    d = fresh(); d.two.one.n_taps = 17
    refused(d, '1..16 taps')
    d = fresh(); d.cls[1].src2 = 1; d.two.a2_hi = d.two.a2_lo = p; d.two.k2 = 64      # a second source on class 1
    refused(d, 'class 0 only')
    d = fresh(); d.cls[0].src2 = 1                                         # ... on class 0 without its planes
    refused(d, 'class 0 only')
    d = fresh(); d.two.a2_hi = d.two.a2_lo = p; d.two.k2 = 64              # planes that no class takes
    refused(d, 'needs class 0 to take it')
    d = fresh(); d.two.a2_hi = p                                           # half a pair
    refused(d, 'both planes or none')
    d = fresh(); d.cls[3].k_off = 9 * 64 * 2 - 64                          # the slice runs past the row
    refused(d, "class's slice")
    d = fresh(); d.cls[2].k_off += 4                                       # 8-byte aligned only
    refused(d, "class's slice")
    d = fresh(); d.cls[3].dst_oy = 2                                       # row 2 * 2 + 2 = 6 of a 6-row image
    refused(d, 'destination pixel')
    d = fresh(); d.two.one.flags = 16
    refused(d, 'interleaved')
    d = fresh(); d.two.one.conv = 0
    refused(d, 'conv mode only')
    assert lib.rart_gemm_pair_max_classes() == 4 and lib.rart_gemm_pair_max_sources() == 2


def test_class_tables_cpu():
    """(no GPU) the class-ordered tables of a small stride-2 Bottleneck: the 3x3's four per-class tables side by side, and the shortcut's
    [W1^T | Wds^T], W1^T, W1^T, W1^T, each as [hi | lo | hi] rows; the per-class tables and `w_cat_bwd` of a stride-2 block stay as they were."""
    from robustart_amd.model.engine import _Conv, class_tables
    from robustart_amd.model.resnet_torch import Bottleneck
    torch.manual_seed(9)
    cin, planes = 64, 32
    ds = torch.nn.Sequential(torch.nn.Conv2d(cin, 4 * planes, 1, stride=2, bias=False), torch.nn.BatchNorm2d(4 * planes))
    blk = Bottleneck(cin, planes, 2, ds).eval()
    ca, cb, cd = (_Conv(blk.conv1, blk.bn1, 'cpu', split=True), _Conv(blk.conv2, blk.bn2, 'cpu', split=True),
                  _Conv(blk.downsample[0], blk.downsample[1], 'cpu', split=True))
    class_tables(ca, cb, cd)
    tab, cls = cb.cls_bwd
    ktot = 9 * planes
    assert tab.shape == (cb.bwd[0][2].shape[0], 3 * ktot) and [len(t) for t, _, _ in cls] == [1, 2, 2, 4]
    for (taps, off, parity), (p0, t0, w) in zip(cls, cb.bwd):
        k = planes * len(taps)
        assert parity == p0 and taps == t0
        for pl in range(3):
            assert torch.equal(tab[:, pl * ktot + off:pl * ktot + off + k], w[:, pl * k:(pl + 1) * k])
    tab, cls = cd.cls_bwd
    w1, wd = ca.bwd[0][2], cd.bwd[0][2]
    ktot = 4 * planes + 4 * planes
    assert tab.shape == (w1.shape[0], 3 * ktot) and [(t, p) for t, _, p in cls] == [([p], p) for p in PARITIES]
    assert [off for _, off, _ in cls] == [0, planes + 4 * planes, 2 * planes + 4 * planes, 3 * planes + 4 * planes]
    for pl in range(3):
        assert torch.equal(tab[:, pl * ktot:pl * ktot + planes], w1[:, pl * planes:(pl + 1) * planes])
        assert torch.equal(tab[:, pl * ktot + planes:pl * ktot + 5 * planes], wd[:, pl * 4 * planes:(pl + 1) * 4 * planes])
        for _, off, _ in cls[1:]:
            assert torch.equal(tab[:, pl * ktot + off:pl * ktot + off + planes], w1[:, pl * planes:(pl + 1) * planes])
    assert getattr(cd, 'w_cat_bwd', None) is None


@gpu
def test_x3_class_launches_match_the_per_class_chain():
    """Full ResNet-50 at B = 2, 64 x 64, reference precision.  The class launches of the stride-2 3x3 backward alone (no shortcut fold) give
    the per-class chain's input gradient bit for bit; with the stride-2 shortcuts folded into conv1^T's class launch the logits stay
    bit-equal (the forward is untouched) and the gradient moves by one rounding fewer: the bound of
    tests/test_shortcut_fusion_gpu.py for `fused_shortcut_pair` (relative L2 <= 0.15, cosine >= 0.98 per sample)."""
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    torch.manual_seed(0)
    m = randomize_bn_stats(get_model({'type': 'resnet50_official'}), 0).eval().cuda()
    for p in m.parameters():
        p.requires_grad_(False)
    eng = ResNet50Engine(m, 'cuda', precision='fp32x')
    g = torch.Generator().manual_seed(43)
    x = torch.rand(2, 3, 64, 64, generator=g).cuda()
    y = torch.randint(0, 1000, (2,), generator=g).cuda()
    assert eng.pair_class_launch and eng.pair_classes == 4 and eng.fused_shortcut_pair
    s2 = [b for b in eng.blocks if b[1].stride == 2]
    assert len(s2) == 3 and all(getattr(b[1], 'cls_bwd', None) is not None and getattr(b[3], 'cls_bwd', None) is not None for b in s2)

    def run():
        calls = []
        real = eng._launch_pair_classes
        eng._launch_pair_classes = lambda d, nbytes=None: (calls.append(d.n_classes), real(d, nbytes))[1]
        try:
            lo, _, gr, _ = eng.forward_backward(x, MEAN, STD, y, 0)
        finally:
            del eng._launch_pair_classes
        return lo.clone(), gr.clone(), len(calls)
    all_3x3, all_sc = (128, 256, 512), (256, 512, 1024)
    keep = (eng.class_3x3_channels, eng.class_shortcut_channels)
    try:
        eng.class_3x3_channels, eng.class_shortcut_channels = all_3x3, all_sc
        la, ga, na = run()
        eng.class_shortcut_channels = ()
        lb, gb, nb = run()
        eng.pair_class_launch = False
        lc, gc, nc = run()
    finally:
        eng.pair_class_launch = True
        eng.class_3x3_channels, eng.class_shortcut_channels = keep
    assert (na, nb, nc) == (6, 3, 0)
    assert torch.equal(la, lc) and torch.equal(lb, lc)
    assert torch.equal(gb, gc)
    a, b = ga.double().flatten(1), gc.double().flatten(1)
    rel = ((a - b).norm(dim=1) / b.norm(dim=1)).max().item()
    cos = ((a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).min().item()
    print('x3 class launches vs the per-class chain: gradient rel L2 %.2e, cos %.6f' % (rel, cos))
    assert rel <= 0.15 and cos >= 0.98
