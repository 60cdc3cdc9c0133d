"""The shared launch layer (robustart_amd/model/engine_base.py) without a GPU: descriptors built from CPU tensors, field by field,
through the builders and through the engines' adapters with the library call replaced by a recorder."""
import importlib.util
import json
import os

import torch
from _recorder import Recorder as _Recorder

from robustart_amd import _lib
from robustart_amd.model import engine_base as eb


def _engine(cls, monkeypatch, **attrs):
    monkeypatch.setattr(_lib, 'stream_ptr', lambda: None)
    eng = cls.__new__(cls)
    eng.lib, eng.profile, eng._buf, eng._w_il = _Recorder(), None, {}, {}
    for k, v in attrs.items():
        setattr(eng, k, v)
    return eng


def _bf(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


def test_strided_conv_with_per_tap_source_offsets():
    src, wgt, dst = _bf(2, 2, 9, 9, 16), _bf(64, 3 * 16), _bf(2, 4, 4, 64)
    bias, res, sign, stats = torch.zeros(64), _bf(2, 4, 4, 64), torch.zeros(2, 4, 4, 8, dtype=torch.uint8), torch.zeros(512)
    taps = [(0, 0), (0, 1), (1, 0)]
    d = eb.conv_desc(src[0], wgt, dst, 2, (4, 4), (9, 9), 16, 16, taps, 64, (4, 4), 64, bias=bias, res=res, sign_out=sign,
                     stats_out=stats, flags=eb.F_RELU, stride=(2, 2), tap_src_off=[0, 0, eb.lo_off(src)])
    assert (d.src, d.wgt, d.dst) == (src.data_ptr(), wgt.data_ptr(), dst.data_ptr())
    assert (d.bias, d.res, d.sign_out, d.bn_stats_out, d.mask) == (bias.data_ptr(), res.data_ptr(), sign.data_ptr(), stats.data_ptr(), None)
    assert (d.batch, d.grid_h, d.grid_w, d.src_h, d.src_w, d.src_pix_stride) == (2, 4, 4, 9, 9, 16)
    assert (d.k_per_tap, d.n_taps, d.sy, d.sx, d.n_cols, d.flags) == (16, 3, 2, 2, 64, eb.F_RELU)
    assert [(d.tap_dy[i], d.tap_dx[i]) for i in range(3)] == taps
    assert list(d.tap_src_off[:4]) == [0, 0, 2 * 9 * 9 * 16, 0]
    assert (d.dst_h, d.dst_w, d.dst_sy, d.dst_sx, d.dst_oy, d.dst_ox, d.dst_pix_stride) == (4, 4, 1, 1, 0, 0, 64)
    assert (d.n_batched, d.dst_pair_off, d.res_pair_off) == (0, 0, 0)


def test_vit_batched_row_product(monkeypatch):
    """S = Q K^T per (image, head) on the conv descriptor: ViT's call, B = 2 images, H = 3 heads of hd = 32, T = 10 tokens"""
    from robustart_amd.model.vit_engine import ViTEngine
    eng = _engine(ViTEngine, monkeypatch)
    B, H, hd, T = 2, 3, 32, 10
    D, s_ld = H * hd, 16
    qkv, scores = _bf(B * T, 3 * D), _bf(B * H, T, s_ld)
    eng._gemm(qkv, qkv[:, D:], scores, T, hd, s_ld, 3 * D, s_ld, rows_per_image=T,
              batched=dict(n=B * H, inner=H, src=(T * 3 * D, hd), wgt=(T * 3 * D, hd), dst=(H * T * s_ld, T * s_ld), wgt_row_stride=3 * D))
    d, = eng.lib.descs
    assert (d.src, d.wgt, d.dst) == (qkv.data_ptr(), qkv.data_ptr() + 2 * D, scores.data_ptr())
    assert (d.batch, d.grid_h, d.grid_w, d.src_h, d.src_w, d.src_pix_stride) == (1, T, 1, T, 1, 3 * D)
    assert (d.k_per_tap, d.n_taps, d.n_cols, d.dst_h, d.dst_w, d.dst_pix_stride, d.flags) == (hd, 1, s_ld, T, 1, s_ld, 0)
    assert (d.n_batched, d.z_inner, d.wgt_row_stride) == (B * H, H, 3 * D)
    assert (d.src_z_outer, d.src_z_inner, d.wgt_z_outer, d.wgt_z_inner) == (T * 3 * D, hd, T * 3 * D, hd)
    assert (d.dst_z_outer, d.dst_z_inner) == (H * T * s_ld, T * s_ld)


def _resnet_pair(monkeypatch, interleaved):
    from robustart_amd.model.engine import ResNet50Engine
    eng = _engine(ResNet50Engine, monkeypatch, pair_w_interleaved=interleaved, pair_tile=(0, 0), pair_gemm_kernel=True)
    K, n = 9 * 32, 64
    src, dst, res = _bf(2, 2, 6, 6, 32), _bf(2, 2, 6, 6, n), _bf(2, 2, 6, 6, n)
    wgt = torch.arange(n * 3 * K, dtype=torch.float32).reshape(n, 3 * K).to(torch.bfloat16)     # [rows][hi | lo | hi]
    mask, bias = torch.zeros(2, 6, 6, n // 8, dtype=torch.uint8), torch.zeros(n)
    taps = [(r - 1, s - 1) for r in range(3) for s in range(3)]
    eng._gemm(src, wgt, dst, 2, (6, 6), (6, 6), 32, 32, taps, n, (6, 6), n, bias=bias, res=res, mask=mask, flags=eb.F_RELU, pair=True)
    d, = eng.lib.descs
    assert (d.a_hi, d.a_lo) == (src[0].data_ptr(), src[1].data_ptr())
    assert (d.dst_hi, d.dst_lo, d.res_hi, d.res_lo) == (dst[0].data_ptr(), dst[1].data_ptr(), res[0].data_ptr(), res[1].data_ptr())
    assert (d.bias, d.mask_bits, d.sign_out, d.aux_hi) == (bias.data_ptr(), mask.data_ptr(), None, None)
    assert (d.conv, d.batch, d.grid_h, d.grid_w, d.src_h, d.src_w, d.k_per_tap, d.n_taps) == (1, 2, 6, 6, 6, 6, 32, 9)
    assert [(d.tap_dy[i], d.tap_dx[i]) for i in range(9)] == taps
    assert (d.M, d.N, d.K, d.lda, d.ldc, d.w_rows) == (72, n, K, 32, n, n)
    return eng, d, wgt, K


def test_pair_launch_from_a_hi_lo_hi_table(monkeypatch):
    eng, d, wgt, K = _resnet_pair(monkeypatch, False)
    assert (d.w_hi, d.w_lo, d.ldw, d.flags) == (wgt.data_ptr(), wgt.data_ptr() + 2 * K, 3 * K, eb.GP_RELU)


def test_pair_launch_on_the_interleaved_weight_copy(monkeypatch):
    eng, d, wgt, K = _resnet_pair(monkeypatch, True)
    il = eng._w_il[wgt.data_ptr()]
    assert (d.w_hi, d.w_lo, d.ldw, d.flags) == (il.data_ptr(), il.data_ptr() + 64, 2 * K, eb.GP_RELU | eb.GP_W_INTERLEAVED)
    assert eb.GP_W_INTERLEAVED == 16
    # per row and 32-deep K step: the hi slice, then the lo slice
    assert torch.equal(il[:, :32], wgt[:, :32]) and torch.equal(il[:, 32:64], wgt[:, K:K + 32]) and torch.equal(il[:, 64:96], wgt[:, 32:64])


def test_pair_plane_offsets_and_fp32_destination(monkeypatch):
    """dK = dS^T Q of ViT's unfused attention backward (plane offsets of a column slice) and a product into an fp32 matrix"""
    from robustart_amd.model.vit_engine import ViTEngine
    eng = _engine(ViTEngine, monkeypatch)
    M, N, K, ld = 16, 32, 64, 96
    a, w, dst = _bf(2, M, ld), _bf(2, N, ld), _bf(2, M, 3 * ld)
    eng._gemm_pair(a, w, dst, M, N, K, ld, 3 * ld, ldw=ld, w_rows=N, a_off=8, w_off=32, dst_off=ld)
    out = torch.zeros(M, N)
    eng._gemm_pair(a, w, out, M, N, K, ld, N, ldw=ld, flags=eb.GP_OUT_F32, aux=None)
    d, f = eng.lib.descs
    assert (d.a_hi, d.a_lo) == (a[0].data_ptr() + 16, a[1].data_ptr() + 16)
    assert (d.w_hi, d.w_lo) == (w[0].data_ptr() + 64, w[1].data_ptr() + 64)
    assert (d.dst_hi, d.dst_lo) == (dst[0].data_ptr() + 2 * ld, dst[1].data_ptr() + 2 * ld)
    assert (d.M, d.N, d.K, d.lda, d.ldw, d.ldc, d.w_rows, d.flags, d.conv) == (M, N, K, ld, ld, 3 * ld, N, 0, 0)
    assert (f.dst_hi, f.dst_lo, f.flags, f.ldc, f.w_rows) == (out.data_ptr(), None, eb.GP_OUT_F32, N, N)
    # the fp32 destination's element offset is in 4-byte elements
    g = eb.gemm_pair_desc(a, w, out, N, ld, ld, N, N, M=M, K=K, flags=eb.GP_OUT_F32, dst_off=5)
    assert g.dst_hi == out.data_ptr() + 20


def test_pair_table_helpers():
    t = torch.randn(5, 70)
    hi, lo = eb.split_hi_lo(t)
    assert torch.equal(hi, t.to(torch.bfloat16)) and torch.equal(lo, (t - hi.float()).to(torch.bfloat16))
    p = eb.pair(t)
    assert p.shape == (2, 5, 70) and p.is_contiguous() and eb.lo_off(p) == 5 * 70
    w = eb.pad_rows(eb.pad_k(t, 96), 64)
    assert w.shape == (64, 96) and w.is_contiguous() and torch.equal(w[:5, :70], t) and not w[5:].any() and not w[:, 70:].any()
    assert eb.pad_k(t, None) is t and eb.rows_mult(64) == 64 and eb.rows_mult(65) == 128
    assert list(eb.cints([])) == [0] and list(eb.cints([3, -1])) == [3, -1]


def test_weight_gradient_splits():
    """the split-K heuristics of both weight-gradient paths at pinned shapes: a change to either changes the launches of the train engines"""
    direct = {(802816, 64, 9, 64): (204, 3936), (6272, 2048, 1, 512): (16, 416), (802816, 4, 49, 64): (512, 1568),
              (256, 1024, 1, 1024): (1, 256), (50176, 128, 4, 256): (121, 416)}
    for (M, x_c, taps, n), want in direct.items():
        splits, chunk = eb.wgrad_split_direct(M, x_c, taps, n, 1024, 256)
        assert (splits, chunk) == want and chunk % 32 == 0 and (splits - 1) * chunk < M <= splits * chunk
    transposed = {(197 * 256, 768, 768): (28, 1856, 768), (8, 2048, 1000): (1, 64, 1024), (8, 48, 48): (1, 64, 64),
                  (197 * 256, 3072, 768): (7, 7232, 768)}
    for args, want in transposed.items():
        assert eb.wgrad_split_transposed(*args) == want


def test_precision_table():
    assert eb.check_precision('fp32x') == eb.check_precision('bf16x3') == 'bf16x3' and eb.check_precision('bf16') == 'bf16'
    try:
        eb.check_precision('fp16')
    except ValueError as e:
        assert 'precision must be one of' in str(e)
    else:
        raise AssertionError('fp16 accepted')


# ---------------------------------------------------------------------- the precision-generic launches of RowEngine, and ViT's one chain
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _vit(monkeypatch, precision, depth=1):
    """ViTEngine on the CPU: 32 px, 4 patches + class token, 2 heads of 64, tables built by refold"""
    from robustart_amd.model.vit_engine import ViTEngine
    from robustart_amd.model.vit_torch import VisionTransformer
    torch.manual_seed(0)
    m = VisionTransformer(img_size=32, num_classes=10, embed_dim=128, depth=depth, num_heads=2).eval()
    monkeypatch.setattr(_lib, 'require_gpu', lambda: torch)
    eng = _engine(ViTEngine, monkeypatch, device=torch.device('cpu'), precision=eb.check_precision(precision), D=128, H=2, ps=16, hd=64,
                  pair_w_interleaved=False, fused_attention=True, fused_attention_bwd=True)
    eng.refold(m)
    return eng


def _vals(args):
    return tuple(a.value if hasattr(a, 'value') else a for a in args)


def _planes(t, x3):
    return (t[0].data_ptr(), t[1].data_ptr()) if x3 else (t.data_ptr(),)


def _kinds(eng):
    """entry names with the precision taken out; the per-plane transposes of the pair decomposition count once"""
    out = []
    for name, _ in eng.lib.calls:
        if name in ('rart_conv_igemm_bf16', 'rart_gemm_pair_bf16'):
            name = 'gemm'
        else:
            name = name.replace('_pair', '').replace('_bf16', '').replace('unpatchify_from_f32', 'unpatchify_f32')
        if not (out and out[-1] == name and name in ('rart_vit_transpose_v', 'rart_transpose_gather')):
            out.append(name)
    eng.lib.calls.clear()
    return out


def test_x3_is_a_property_of_the_precision(monkeypatch):
    eng = _engine(eb.RowEngine, monkeypatch, precision='bf16')
    assert eng.x3 is False
    eng.precision = eb.check_precision('fp32x')
    assert eng.x3 is True
    assert [eb.k32(n) for n in (1, 32, 33, 197, 1000)] == [32, 32, 64, 224, 1024]


def test_vit_chain_launches_the_same_sequence_in_both_precisions(monkeypatch):
    """forward and forward + backward of a one-block ViT: entry for entry the same chain, up to the per-precision details"""
    from robustart_amd.noise import adv
    B, T, D = 2, 5, 128
    x = torch.rand(B, 3, 32, 32)
    monkeypatch.setattr(adv, 'logit_loss', lambda logits, *a: (torch.zeros(B), torch.ones(B, 10), torch.zeros(B, dtype=torch.int32)))
    bf, x3 = _vit(monkeypatch, 'bf16'), _vit(monkeypatch, 'fp32x')
    bf.lib.gemm256 = 1
    for fused in (True, False):
        for e in (bf, x3):
            e.fused_attention = e.fused_attention_bwd = fused
        bf.logits(x, MEAN, STD), x3.logits(x, MEAN, STD)
        fwd = _kinds(bf)
        assert fwd == _kinds(x3)
        assert fwd[:3] == ['rart_vit_patchify', 'gemm', 'rart_vit_add_pos_cls'] and fwd[-2:] == ['rart_layernorm', 'gemm']
        assert ('rart_vit_attention' in fwd) == fused and ('rart_softmax_rows' in fwd) == (not fused)
        bf.forward_backward(x, MEAN, STD, None, 0), x3.forward_backward(x, MEAN, STD, None, 0)
        both = _kinds(bf)
        assert both == _kinds(x3)
        assert both[:len(fwd)] == fwd and both[-2:] == ['gemm', 'rart_vit_unpatchify_f32']
        assert ('rart_vit_attention_bwd' in both) == fused and ('rart_softmax_bwd_rows' in both) == (not fused)
    # bf16 only: where the 256 x 256 GEMM does not take fc1, the pre-activation is kept by a GEMM and rart_gelu_bf16 follows
    bf.lib.gemm256 = 0
    bf.forward_backward(x, MEAN, STD, None, 0)
    two = _kinds(bf)
    i = two.index('rart_gelu')
    assert two[:i] + two[i + 1:] == both
    # the per-precision details
    assert tuple(bf._buf['qkv0'].shape) == (B * T + 256, 3 * D) and tuple(x3._buf['qkv0'].shape) == (2, B * T, 3 * D)
    bf.forward_backward(x, MEAN, STD, None, 0), x3.forward_backward(x, MEAN, STD, None, 0)
    assert 'att_stats' not in bf._buf                                        # the pair fused backward only
    assert tuple(x3._buf['att_stats'].shape) == (B * 2, 32, 4) and x3._buf['att_stats'].dtype == torch.float32
    pe_x3, dg_x3 = x3.lib.descs[0], x3.lib.descs[-1]
    pe_bf, dg_bf = bf.lib.descs[0], bf.lib.descs[-1]
    # patch GEMM: the image pair as two taps of the [hi | hi] table, or the pair GEMM on the pair; rows 1 .. T-1 of every image
    assert (pe_bf.n_taps, pe_bf.tap_src_off[1], pe_bf.src) == (2, eb.lo_off(bf._buf['patches']), bf._buf['patches'].data_ptr())
    assert (pe_bf.batch, pe_bf.grid_h, pe_bf.dst_h, pe_bf.dst_oy) == (B, T - 1, T, 1)
    assert (pe_x3.a_hi, pe_x3.a_lo) == _planes(x3._buf['patches'], True)
    assert (pe_x3.rows_per_image, pe_x3.dst_rows_per_image, pe_x3.dst_row_off, pe_x3.src_row_off) == (T - 1, T, 1, 0)
    # patch dgrad: from token row 1 of every image, into bf16 / fp32 patches
    dx = bf._buf['g_x_a']
    assert (dg_bf.src, dg_bf.batch, dg_bf.grid_h, dg_bf.src_h, dg_bf.flags) == (dx.data_ptr() + 2 * D, B, T - 1, T, 0)
    assert bf._buf['g_patch'].dtype == torch.bfloat16
    assert (dg_x3.a_hi, dg_x3.a_lo) == _planes(x3._buf['g_x_a'], True) and dg_x3.flags == eb.GP_OUT_F32
    assert (dg_x3.rows_per_image, dg_x3.src_rows_per_image, dg_x3.src_row_off, dg_x3.dst_rows_per_image) == (T - 1, T, 1, 0)
    assert x3._buf['g_patch'].dtype == torch.float32
    assert x3.lib.calls[-1][0] == 'rart_vit_unpatchify_from_f32' and bf.lib.calls[-1][0] == 'rart_vit_unpatchify_f32'


def test_layernorm_launches_with_class_token_strides(monkeypatch):
    """ViT's head reads the class-token row of every image: B rows T * D apart, forward and backward; the default is dense"""
    B, T, D = 3, 5, 128
    for prec in ('bf16', 'bf16x3'):
        eng = _engine(eb.RowEngine, monkeypatch, precision=prec)
        x3 = eng.x3

        def act(*shape):
            return _bf(*(((2,) if x3 else ()) + shape))
        x, cls, dcls, dx, res = act(B, T, D), act(B, D), act(B, D), act(B, T, D), act(B, T, D)
        g, b = torch.zeros(D), torch.zeros(D)
        eng._ln(x, g, b, cls, B, D, ld_in=T * D)
        eng._ln_bwd(dcls, x, g, None, dx, B, D, strides=(D, T * D, 0, T * D))
        eng._ln(x, g, b, dx, B * T, D)
        eng._ln_bwd(dx, x, g, res, dx, B * T, D)
        eng._ln_bwd(dx, x, g, None, dx, B * T, D)
        (n0, a0), (n1, a1), (n2, a2), (n3, a3), (n4, a4) = eng.lib.calls
        sfx = 'pair' if x3 else 'bf16'
        assert [n0, n1, n2, n3, n4] == ['rart_layernorm_' + sfx, 'rart_layernorm_bwd_' + sfx] + ['rart_layernorm_' + sfx] + \
            ['rart_layernorm_bwd_' + sfx] * 2
        no_res = (None, None) if x3 else (None,)
        assert _vals(a0) == _planes(x, x3) + (g.data_ptr(), b.data_ptr()) + _planes(cls, x3) + (B, D, T * D, D, 1e-6, None)
        assert _vals(a1) == _planes(dcls, x3) + _planes(x, x3) + (g.data_ptr(),) + no_res + _planes(dx, x3) + \
            (B, D, D, T * D, 0, T * D, 1e-6, None)
        assert _vals(a2) == _planes(x, x3) + (g.data_ptr(), b.data_ptr()) + _planes(dx, x3) + (B * T, D, D, D, 1e-6, None)
        assert _vals(a3) == _planes(dx, x3) + _planes(x, x3) + (g.data_ptr(),) + _planes(res, x3) + _planes(dx, x3) + \
            (B * T, D, D, D, D, D, 1e-6, None)
        assert _vals(a4) == _planes(dx, x3) + _planes(x, x3) + (g.data_ptr(),) + no_res + _planes(dx, x3) + (B * T, D, D, D, 0, D, 1e-6, None)


def test_fc1_gelu_forms(monkeypatch):
    """bf16: GELU in the epilogue; with the pre-activation kept, one launch where the 256 x 256 GEMM takes the shape, else the GEMM
    into u and rart_gelu_bf16.  Pair: always one launch."""
    rows, K, N = 64, 128, 512
    w, wp, b = _bf(N, K), _bf(2, N, K), torch.zeros(N)
    ln, hid, u = _bf(rows, K), _bf(rows, N), _bf(rows, N)
    eng = _engine(eb.RowEngine, monkeypatch, precision='bf16')
    eng._fc1_gelu(ln, w, b, hid, None, rows, K, N, False)
    eng.lib.gemm256 = 1
    eng._fc1_gelu(ln, w, b, hid, u, rows, K, N, True)
    eng.lib.gemm256 = 0
    eng._fc1_gelu(ln, w, b, hid, u, rows, K, N, True)
    assert [n for n, _ in eng.lib.calls] == ['rart_conv_igemm_bf16'] * 3 + ['rart_gelu_bf16']
    plain, keep, two = eng.lib.descs
    assert (plain.src, plain.wgt, plain.bias, plain.dst, plain.mask, plain.flags) == \
        (ln.data_ptr(), w.data_ptr(), b.data_ptr(), hid.data_ptr(), None, eb.F_GELU)
    assert (plain.batch, plain.grid_h, plain.k_per_tap, plain.n_cols, plain.src_pix_stride, plain.dst_pix_stride) == (1, rows, K, N, K, N)
    assert (keep.dst, keep.mask, keep.flags) == (hid.data_ptr(), u.data_ptr(), eb.F_GELU_KEEP)
    assert (two.dst, two.mask, two.bias, two.flags) == (u.data_ptr(), None, b.data_ptr(), 0)
    assert _vals(eng.lib.calls[-1][1]) == (u.data_ptr(), hid.data_ptr(), rows * N, None)
    lnp, hidp, up = _bf(2, rows, K), _bf(2, rows, N), _bf(2, rows, N)
    eng = _engine(eb.RowEngine, monkeypatch, precision='bf16x3')
    eng._fc1_gelu(lnp, wp, b, hidp, None, rows, K, N, False)
    eng._fc1_gelu(lnp, wp, b, hidp, up, rows, K, N, True)
    assert [n for n, _ in eng.lib.calls] == ['rart_gemm_pair_bf16'] * 2
    plain, keep = eng.lib.descs
    assert (plain.flags, plain.aux_hi, plain.aux_lo) == (eb.GP_GELU, None, None)
    assert (keep.flags, keep.aux_hi, keep.aux_lo) == (eb.GP_GELU_KEEP,) + _planes(up, True)
    for d in (plain, keep):
        assert (d.a_hi, d.a_lo, d.w_hi, d.w_lo, d.dst_hi, d.dst_lo) == _planes(lnp, True) + _planes(wp, True) + _planes(hidp, True)
        assert (d.M, d.N, d.K, d.lda, d.ldw, d.ldc, d.bias) == (rows, N, K, K, K, N, b.data_ptr())


def test_vit_tables_exist_in_the_engines_precision_only(monkeypatch):
    """every Linear table (patch embedding, qkv, proj, fc1, fc2, head; forward and backward-to-input) is a pair [2][rows][K] in
    reference precision and a bf16 [rows][K] matrix in bf16: an engine holds no table of the other precision"""
    names = ['qkv_w', 'proj_w', 'fc1_w', 'fc2_w', 'qkv_wd', 'proj_wd', 'fc1_wd', 'fc2_wd']
    for prec, dims in (('bf16', 2), ('fp32x', 3)):
        eng = _vit(monkeypatch, prec, depth=2)
        tabs = [eng.pe_w, eng.pe_wd, eng.head_w, eng.head_wd] + [L[n] for L in eng.layers for n in names]
        assert len(tabs) == 20
        held = [t for t in vars(eng).values() if torch.is_tensor(t)] + [t for L in eng.layers for t in L.values() if torch.is_tensor(t)]
        bf16 = [t for t in held if t.dtype == torch.bfloat16]
        assert len(bf16) == len(tabs) and {t.data_ptr() for t in bf16} == {t.data_ptr() for t in tabs}
        for t in tabs:
            assert t.dim() == dims and t.is_contiguous() and (dims == 2 or t.shape[0] == 2)
            assert t.shape[-2] % (256 if dims == 3 else 64) == 0
        assert not isinstance(eng.x3, dict)
        # same keys in both precisions
        assert sorted(k for k in eng.layers[0] if k.endswith(('_w', '_wd'))) == sorted(names)


# ---------------------------------------------------------------------- ResNet-50's one chain
_RESNET = []


def _resnet_model():
    from robustart_amd.model import get_model
    if not _RESNET:
        torch.manual_seed(0)
        _RESNET.append(get_model({'type': 'resnet50_official'}).eval())
    return _RESNET[0]


def _cpu_library(monkeypatch, supported):
    """the recorder as the library of engines built on the CPU by their own constructors"""
    rec = _Recorder()
    rec.supported = supported
    monkeypatch.setattr(_lib, 'require_gpu', lambda: torch)
    monkeypatch.setattr(_lib, 'stream_ptr', lambda: None)
    monkeypatch.setattr(_lib, 'load', lambda: rec)
    return rec


def _resnet(monkeypatch, precision, supported=lambda name, args: 0):
    """ResNet50Engine of the full (3, 4, 6, 3) network on the CPU; supported(name, args) answers every rart_*_supported"""
    from robustart_amd.model.engine import ResNet50Engine
    rec = _cpu_library(monkeypatch, supported)
    eng = ResNet50Engine(_resnet_model(), 'cpu', precision)
    rec.calls.clear()
    return eng


def _stub_loss(monkeypatch, B, n=1000):
    from robustart_amd.noise import adv
    monkeypatch.setattr(adv, 'logit_loss', lambda logits, *a: (torch.zeros(B), torch.ones(B, n), torch.zeros(B, dtype=torch.int32)))


def _names(eng):
    out = [n for n, _ in eng.lib.calls]
    eng.lib.calls.clear()
    return out


def _resnet_kinds(eng):
    """entry names with the precision taken out; every GEMM launcher reads as 'gemm'"""
    out = []
    for n in _names(eng):
        n = n.replace('_pair', '').replace('_bf16', '')
        out.append('gemm' if n in ('rart_conv_igemm', 'rart_gemm', 'rart_gemm_small_m') else n)
    return out


def test_resnet_chain_launches_the_same_sequence_in_both_precisions(monkeypatch):
    """with no fused block kernel available, forward and forward + backward are entry for entry the same chain in bf16 and in
    reference precision: stem, 52 convolutions, pool, classifier, and back"""
    B = 2
    x = torch.rand(B, 3, 64, 64)
    _stub_loss(monkeypatch, B)
    bf, x3 = _resnet(monkeypatch, 'bf16'), _resnet(monkeypatch, 'fp32x')
    bf.logits(x, MEAN, STD), x3.logits(x, MEAN, STD)
    fwd = _resnet_kinds(bf)
    assert fwd == _resnet_kinds(x3)
    assert len(fwd) == 55 and fwd == ['rart_engine_stem_fwd_fused'] + ['gemm'] * 52 + ['rart_engine_avgpool', 'gemm']
    u8 = torch.zeros(B, 64, 64, 3, dtype=torch.uint8)
    bf.logits_from_u8(u8, MEAN, STD), x3.logits_from_u8(u8, MEAN, STD)
    assert _resnet_kinds(bf) == fwd == _resnet_kinds(x3)
    bf.forward_backward(x, MEAN, STD, None, 0), x3.forward_backward(x, MEAN, STD, None, 0)
    both = _resnet_kinds(bf)
    assert both == _resnet_kinds(x3)
    assert len(both) == 120 and both.count('gemm') == 115 and both[:55] == fwd
    # a 1x1 / 2 projection reaches one input-parity class, a 3x3 / 2 all four: 52 + 3 * 3 backward convolutions, one classifier
    assert both[55:] == ['rart_f32_to_rows', 'gemm', 'rart_engine_avgpool_bwd'] + ['gemm'] * 61 + ['rart_engine_stem_bwd_fused']
    # the per-precision details: activations and gradients are bf16 tensors or pairs under the same names
    for name in ('p1', 'b0_a', 'b0_b', 'b0_c', 'b0_ds', 'b15_c', 'pooled', 'g_dl', 'dpool', 'g_a', 'g_out_-1', 'g_out_15'):
        assert tuple(x3._buf[name].shape) == (2,) + tuple(bf._buf[name].shape), name
    assert 'g_b' in bf._buf and 'g_b0' not in bf._buf and 'g_b' not in x3._buf and 'g_b0' in x3._buf and 'g_b1' in x3._buf
    assert not [k for k in list(bf._buf) + list(x3._buf) if k.startswith('x3_')]
    for e in (bf, x3):
        acts = e.last_acts
        assert set(acts) >= {'b0', 'b15', 'b0_masks', 'b15_masks', 'p1', 'y1', 'p1_argmax', 'last', 'in_shape'}
        assert acts['y1'] is None and acts['p1'] is e._buf['p1'] and acts['in_shape'] == (B, 64, 64) and acts['last'][0] is e._buf['b15_c']
        assert all(m.dtype == torch.uint8 for m in acts['b7_masks']) and acts['b7_masks'][1] is e._buf['b7_a_sign']


def _fused_calls(eng):
    return [n for n in _names(eng) if 'bottleneck' in n or 'tail' in n]


def test_resnet_fused_block_dispatch_order_bf16(monkeypatch):
    """one ordered dispatch per block and direction: bottleneck_fused, then the image-resident kernels (14, 28, 7), then
    bottleneck_first, then the stride-2 kernel; the backward takes the same kernels in reverse block order"""
    B = 1
    x = torch.rand(B, 3, 64, 64)
    _stub_loss(monkeypatch, B)
    off = set()
    eng = _resnet(monkeypatch, 'bf16', lambda name, args: int(name not in off))
    fu, fi, s2f, s2b = 'rart_bottleneck_fused_bf16', 'rart_bottleneck_first_bf16', 'rart_bottleneck_s2_fwd_bf16', 'rart_bottleneck_s2_bwd_bf16'

    def image(k):
        return 'rart_bottleneck%d_fused_bf16' % k
    # everything available: every identity block on bottleneck_fused (its check comes first); layer4's first block conv by conv
    fwd = [fi, fu, fu, s2f, fu, fu, fu, s2f] + [fu] * 5 + [fu, fu]
    eng.logits(x, MEAN, STD)
    assert _fused_calls(eng) == fwd
    eng.forward_backward(x, MEAN, STD, None, 0)
    assert _fused_calls(eng) == fwd + [s2b if n == s2f else n for n in reversed(fwd)]
    # without bottleneck_fused: layer2 / layer3 / layer4 identity blocks on the first image-resident kernel that takes the geometry
    for gone, k in ((('rart_bottleneck_fused_supported',), 14), (('rart_bottleneck14_fused_supported',), 28),
                    (('rart_bottleneck28_fused_supported',), 7)):
        off.update(gone)
        fwd = [fi, s2f] + [image(k)] * 3 + [s2f] + [image(k)] * 5 + [image(k)] * 2
        eng.forward_backward(x, MEAN, STD, None, 0)
        assert _fused_calls(eng) == fwd + [s2b if n == s2f else n for n in reversed(fwd)]
    # the switches: 28 and 7 behind their own and behind fused_bottleneck14; the stride-2 backward behind its own
    eng.fused_bottleneck7 = False
    eng.fused_bottleneck_s2_bwd = False
    eng.forward_backward(x, MEAN, STD, None, 0)
    assert _fused_calls(eng) == [fi, s2f, s2f, fi]
    eng.fused_bottleneck7, eng.fused_bottleneck14, eng.fused_bottleneck_s2, eng.fused_bottleneck = True, False, False, False
    eng.forward_backward(x, MEAN, STD, None, 0)
    assert _fused_calls(eng) == []
    # the fused kernels emit and read 1-bit masks only: with the bf16 activations as masks (cross-check) they serve the inference forward alone
    off.clear()
    eng.fused_bottleneck14 = eng.fused_bottleneck_s2 = eng.fused_bottleneck = True
    eng.sign_bit_masks = False
    eng.forward_backward(x, MEAN, STD, None, 0)
    assert _fused_calls(eng) == []
    assert all(a is b for a, b in zip(eng.last_acts['b1_masks'], (eng._buf['b0_c'], eng._buf['b1_a'], eng._buf['b1_b'])))
    eng.logits(x, MEAN, STD)
    assert len(_fused_calls(eng)) == 15


def _tail_descs(eng):
    return [a[0]._obj for n, a in eng.lib.calls if n == 'rart_conv3x3_tail_pair']


def test_resnet_pair_tail_kernel_and_its_hand_over(monkeypatch):
    """reference precision: layer1's 3x3 + 1x1 as one launch; its rider computes the neighbouring block's 1x1 reduction, and that
    block then launches none of its own (forward: conv1 of block bi + 1; backward: conv3^T of block bi - 1)"""
    B = 2
    x = torch.rand(B, 3, 64, 64)
    _stub_loss(monkeypatch, B)
    eng = _resnet(monkeypatch, 'fp32x', lambda name, args: 1)
    tail = 'rart_conv3x3_tail_pair'

    def writers(buf):
        """the GEMM launches that write pair buffer `buf`"""
        return [d for d in eng.lib.descs if d.dst_hi == eng._buf[buf][0].data_ptr()]
    eng.logits(x, MEAN, STD)
    t = _tail_descs(eng)
    assert len(t) == 3 and [d.c_mid for d in t] == [64] * 3 and len(eng.lib.calls) == 55 - 3 - 2
    # blocks 0 and 1 carry conv1 of blocks 1 and 2; block 2's neighbour (layer2, 128 wide) has no rider table
    assert [d.dstn_hi for d in t] == [eng._buf['b1_a'][0].data_ptr(), eng._buf['b2_a'][0].data_ptr(), None]
    assert [d.relu_next for d in t] == [1, 1, 0] and t[0].n_hi == eng.blocks[1][0].next_fwd[0].data_ptr()
    assert len(writers('b0_a')) == 1 and not writers('b1_a') and not writers('b2_a') and len(writers('b3_a')) == 1
    assert 'b0_b' not in eng._buf and 'b3_b' in eng._buf          # the 3x3's output never exists in HBM
    eng.lib.calls.clear()
    eng.forward_backward(x, MEAN, STD, None, 0)
    t = _tail_descs(eng)
    assert len(t) == 5 and [n for n, _ in eng.lib.calls].count(tail) == 5
    fwd, bwd = t[:3], t[3:]
    assert [d.sign_next for d in fwd] == [eng._buf['b1_a_sign'].data_ptr(), eng._buf['b2_a_sign'].data_ptr(), None]
    # backward: blocks 2 and 1 (identity blocks) on the tail kernel, each with conv3^T of the block below into the other g_b buffer
    assert [d.dst_hi for d in bwd] == [eng._buf['g_out_1'][0].data_ptr(), eng._buf['g_out_0'][0].data_ptr()]
    assert [d.dstn_hi for d in bwd] == [eng._buf['g_b1'][0].data_ptr(), eng._buf['g_b0'][0].data_ptr()]
    assert [d.mask_next for d in bwd] == [eng._buf['b1_b_sign'].data_ptr(), eng._buf['b0_b_sign'].data_ptr()]

    def conv3_t(bi):
        """the GEMM launches of conv3^T of block bi"""
        return [d for d in eng.lib.descs if d.w_hi == eng.blocks[bi][2].bwd[0][2].data_ptr()]
    assert not conv3_t(0) and not conv3_t(1) and len(conv3_t(2)) == 1
    with_rider = len(eng.lib.calls)
    # without the rider every block launches its own reduction again: two more in the forward, two more in the backward
    eng.fused_next_pair = False
    eng.lib.calls.clear()
    eng.forward_backward(x, MEAN, STD, None, 0)
    assert len(eng.lib.calls) == with_rider + 4 and all(d.dstn_hi is None and d.n_hi is None for d in _tail_descs(eng))
    assert len(writers('b1_a')) == 1 and len(writers('b2_a')) == 1 and [len(conv3_t(bi)) for bi in range(3)] == [1, 1, 1]
    eng.fused_next_pair = True
    # the backward rider is dropped when the block below kept no mask for it: that block launches its conv3^T itself
    acts, dl = dict(eng.last_acts), eng.last_dlogits
    acts['b1_masks'] = acts['b1_masks'][:2] + (None,)
    eng.lib.calls.clear()
    eng._backward(acts, dl, STD)
    b2, b1 = _tail_descs(eng)
    assert (b2.dstn_hi, b2.n_hi, b2.mask_next) == (None, None, None) and b1.dstn_hi == eng._buf['g_b0'][0].data_ptr()
    own, = conv3_t(1)
    assert own.mask_bits is None and own.dst_hi == eng._buf['g_b1'][0].data_ptr() and not conv3_t(0)
    # the switches of the tail kernel
    eng.fused_tail_channels = (64, 128)
    eng.lib.calls.clear()
    eng.logits(x, MEAN, STD)
    assert [d.c_mid for d in _tail_descs(eng)] == [64] * 3 + [128] * 3
    eng.fused_tail_pair = False
    eng.lib.calls.clear()
    eng.logits(x, MEAN, STD)
    assert not _tail_descs(eng) and len(eng.lib.calls) == 55


def test_resnet_tables_exist_in_the_engines_precision_only(monkeypatch):
    convs = lambda e: [e.stem] + [c for blk in e.blocks for c in blk if c is not None]      # noqa: E731
    bf = _resnet(monkeypatch, 'bf16', lambda name, args: 1)
    x3 = _resnet(monkeypatch, 'fp32x', lambda name, args: 1)
    pair_only = ('stem_w_pair', 'stem_wt_pair')
    assert all(hasattr(x3, n) for n in pair_only) and not any(hasattr(bf, n) for n in pair_only)
    assert hasattr(bf, 'stem_wt') and not hasattr(x3, 'stem_wt')
    frag = ('w_fwd_frag', 'w_bwd_frag', 's2_w1', 's2_w2t', 'bias_sum')
    tails = ('tail_fwd', 'tail_bwd', 'next_fwd', 'next_bwd')
    for names, has, has_not in ((frag, bf, x3), (tails, x3, bf)):
        for n in names:
            assert any(hasattr(c, n) for c in convs(has)) and not any(hasattr(c, n) for c in convs(has_not)), n
    # one table per use, [rows][K] in bf16 and [rows][hi | lo | hi] in reference precision, the same hi plane in both
    for a, b in ((bf.stem_wd, x3.stem_wd), (bf.fc_w, x3.fc_w), (bf.fc_wd, x3.fc_wd), (bf.blocks[3][1].w_fwd, x3.blocks[3][1].w_fwd),
                 (bf.blocks[3][1].bwd[3][2], x3.blocks[3][1].bwd[3][2])):
        k = a.shape[1]
        assert b.shape == (a.shape[0], 3 * k) and torch.equal(b[:, :k], a) and torch.equal(b[:, 2 * k:], a) and a.dtype == b.dtype == torch.bfloat16
    assert bf.stem_w.shape == (64, 448) and torch.equal(bf.stem_w[:, :224], bf.stem_w[:, 224:]) and x3.stem_w.shape == (64, 672)
    assert torch.equal(x3.stem_w[:, :224], bf.stem_w[:, :224]) and torch.equal(x3.stem_w_pair[0], bf.stem_w[:, :224])
    assert torch.equal(x3.stem_w_pair[1], x3.stem_w[:, 224:448])
    w = _RESNET[0].fc.weight.detach()
    assert torch.equal(bf.fc_w[:bf.n_classes], w.to(torch.bfloat16)) and not bf.fc_w[bf.n_classes:].any()
    assert torch.equal(x3.fc_wd[:, 1024:2024], (w - w.to(torch.bfloat16).float()).to(torch.bfloat16).t()) and not x3.fc_wd[:, 1000:1024].any()
    # the precision helpers live on the base class
    assert 'x3' in vars(eb.EngineBase) and all(n in vars(eb.EngineBase) and n not in vars(eb.RowEngine) for n in ('_act', '_hl', '_dlogits_rows'))


# ---------------------------------------------------------------------- the train engine of ResNet-50 and the shared weight gradient
def _resnet_train(monkeypatch, supported=lambda name, args: 1):
    """ResNet50TrainEngine of the full (3, 4, 6, 3) network on the CPU, its constructor's calls still recorded"""
    from robustart_amd.model.train_engine import ResNet50TrainEngine
    m = _resnet_model()
    for p in m.parameters():
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    _cpu_library(monkeypatch, supported)
    return ResNet50TrainEngine(m, 'cpu')


def _counts(eng):
    """recorded launches by entry name (the workspace-size queries are no launches)"""
    out = {}
    for n in _names(eng):
        if not n.endswith('_workspace_bytes'):
            out[n] = out.get(n, 0) + 1
    return out


def test_resnet_train_chain_launch_counts(monkeypatch):
    """constructor, forward and backward of the train engine at 2 x 3 x 64 x 64 with every kernel available: 53 conv + BatchNorm pairs
    and the classifier forward; backward 52 + 9 dgrad launches (a 3x3 / 2 reaches four input parities, a 1x1 / 2 one) + the
    classifier's, and one weight gradient per conv, stem and classifier included, on either weight-gradient path"""
    B = 2
    eng = _resnet_train(monkeypatch)
    assert _counts(eng) == {'rart_pack_jobs_bf16': 1, 'rart_pack_conv_weight_bf16': 1}
    # the stem's row-tap table comes from the eval engine's builder: the image's hi taps, then the same rows for its lo taps
    rows = eb.stem_rows(eng.model.conv1.weight.detach().float()).to(torch.bfloat16)
    assert rows.shape == (64, 224) and torch.equal(eng.stem_w[:, :224], rows) and torch.equal(eng.stem_w[:, 224:], rows)
    x, dl = torch.rand(B, 3, 64, 64), torch.ones(B, 1000)
    fwd = {'rart_engine_prep_input': 1, 'rart_conv_igemm_bf16': 54, 'rart_bn_train_forward_bf16': 53, 'rart_engine_maxpool': 1,
           'rart_engine_avgpool': 1}
    rest = {'rart_f32_to_bf16_rows': 1, 'rart_wgrad_reduce_f32': 54, 'rart_bn_train_backward_bf16': 53, 'rart_engine_avgpool_bwd': 1,
            'rart_engine_maxpool_bwd': 1}
    assert eng.direct_wgrad is True
    eng.forward(x, False, MEAN, STD)
    assert _counts(eng) == fwd
    eng.backward(dl)
    assert _counts(eng) == dict(rest, rart_conv_igemm_bf16=62, rart_wgrad_direct_bf16=54)
    eng.direct_wgrad = False
    eng.forward(x, False, MEAN, STD)
    assert _counts(eng) == fwd
    eng.backward(dl)
    assert _counts(eng) == dict(rest, rart_conv_igemm_bf16=116, rart_transpose_gather_bf16=108)


def test_resnet_train_backward_order_around_an_identity_and_a_projection_block(monkeypatch):
    """per conv: BatchNorm backward, then the weight gradient, then the backward to the input.  Block 15 (identity): the skip gradient
    is formed in conv1's dgrad epilogue from d_out and the sign bits of the block's output; block 13 (layer4's projection block): the
    BatchNorm backward of conv3 writes the masked skip gradient, which the downsample's BatchNorm backward reads"""
    B = 2
    eng = _resnet_train(monkeypatch)
    eng.forward(torch.rand(B, 3, 64, 64), False, MEAN, STD)
    acts = eng.acts
    eng.lib.calls.clear()
    eng.backward(torch.ones(B, 1000))
    calls = eng.lib.calls
    short = {'rart_bn_train_backward_bf16': 'bn', 'rart_wgrad_direct_bf16': 'wgrad', 'rart_wgrad_reduce_f32': 'reduce',
             'rart_conv_igemm_bf16': 'gemm', 'rart_transpose_gather_bf16': 'gather'}
    calls = [(short.get(n, n), a) for n, a in calls if not n.endswith('_workspace_bytes')]
    kinds = [n for n, _ in calls]
    assert kinds[:5] == ['rart_f32_to_bf16_rows', 'wgrad', 'reduce', 'gemm', 'rart_engine_avgpool_bwd']
    conv = ['bn', 'wgrad', 'reduce', 'gemm']
    # blocks 15 and 14: three convs each, one dgrad launch per conv
    assert kinds[5:29] == conv * 6
    b15 = calls[5:17]
    x, xhw, za, ya, zb, yb, zc, zd, out, ohw = acts['b15']
    assert [_vals(a)[3] for n, a in b15 if n == 'bn'] == [zc.data_ptr(), zb.data_ptr(), za.data_ptr()]
    assert _vals(b15[0][1])[5] is None                                   # no skip-gradient tensor
    d_out = _vals(b15[0][1])[0]
    d = b15[-1][1][0]._obj
    assert (d.res, d.mask, d.flags) == (d_out, eng._ysign[out.data_ptr()].data_ptr(), eb.F_MASK_BITS | eb.F_MASK_RES)
    # block 13: conv3, conv2 (3x3 / 2: four parity classes), conv1, then the projection (1x1 / 2: one class)
    assert kinds[29:48] == conv + ['bn', 'wgrad', 'reduce'] + ['gemm'] * 4 + conv + conv
    b13 = calls[29:48]
    x, xhw, za, ya, zb, yb, zc, zd, out, ohw = acts['b13']
    bns = [_vals(a) for n, a in b13 if n == 'bn']
    assert [a[3] for a in bns] == [zc.data_ptr(), zb.data_ptr(), za.data_ptr(), zd.data_ptr()]
    g_skip = bns[0][5]
    assert g_skip is not None and bns[3][:3] == (g_skip, None, 0) and bns[1][5] is None and bns[2][5] is None
    ca_dgrad, ds_dgrad = b13[14][1][0]._obj, b13[18][1][0]._obj
    assert (ca_dgrad.res, ca_dgrad.mask, ca_dgrad.flags) == (None, None, 0)
    assert ds_dgrad.res == ds_dgrad.dst == ca_dgrad.dst and (ds_dgrad.dst_sy, ds_dgrad.dst_sx, ds_dgrad.dst_oy, ds_dgrad.dst_ox) == (2, 2, 0, 0)
    assert [(c[1][0]._obj.dst_oy, c[1][0]._obj.dst_ox) for c in b13[7:11]] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    # the transposing path keeps the order: BatchNorm backward, both transposes, the GEMM, the reduce, then the dgrad
    eng.direct_wgrad = False
    eng.lib.calls.clear()
    eng.backward(torch.ones(B, 1000))
    kinds = [short.get(n, n) for n, _ in eng.lib.calls if not n.endswith('_workspace_bytes')]
    assert kinds[:6] == ['rart_f32_to_bf16_rows', 'gather', 'gather', 'gemm', 'reduce', 'gemm']
    assert kinds[7:7 + 36] == ['bn', 'gather', 'gather', 'gemm', 'reduce', 'gemm'] * 6


def test_train_engine_does_not_read_the_environment(monkeypatch):
    monkeypatch.setenv('RART_TRAIN_FLAGS', 'direct=0')
    assert _resnet_train(monkeypatch).direct_wgrad is True


def _wgrad_calls(eng):
    """(gather of dz, gather of x, GEMM descriptor, reduce) of one weight gradient on the transposing path"""
    (n0, g0), (n1, g1), (n2, mm), (n3, red) = eng.lib.calls
    assert [n0, n1, n2, n3] == ['rart_transpose_gather_bf16'] * 2 + ['rart_conv_igemm_bf16', 'rart_wgrad_reduce_f32']
    taps = [tuple(list(g[i]) for i in (11, 12)) for g in (g0, g1)]
    return [_vals(g[:11] + g[13:]) for g in (g0, g1)], taps, mm[0]._obj, _vals(red)


def _check_wgrad_gemm(eng, d, kp, grid, splits, chunk, n_rows, ld_n):
    dzt, colt, part = (eng._buf[n].data_ptr() for n in ('wg_dzT', 'wg_colT', 'wg_part'))
    assert (d.src, d.wgt, d.dst, d.bias, d.res, d.mask) == (colt, dzt, part, None, None, None)
    assert (d.batch, d.grid_h, d.grid_w) == (1,) + grid and (d.src_h, d.src_w) == grid == (d.dst_h, d.dst_w)
    assert (d.k_per_tap, d.src_pix_stride, d.n_taps, d.tap_dy[0], d.tap_dx[0]) == (chunk, chunk, 1, 0, 0)
    assert (d.n_cols, d.dst_pix_stride, d.flags) == (ld_n, ld_n, eb.F_OUT_F32)
    assert (d.n_batched, d.z_inner, d.wgt_row_stride) == (splits, splits, chunk)
    assert (d.src_z_outer, d.src_z_inner, d.wgt_z_outer, d.wgt_z_inner, d.dst_z_outer, d.dst_z_inner) == \
        (0, kp * chunk, 0, n_rows * chunk, 0, kp * ld_n)
    return dzt, colt, part


def test_shared_weight_gradient_conv_form(monkeypatch):
    """ResNet50TrainEngine._wgrad's transposing path, a 3x3 / 2 conv 64 -> 64 on 2 x 8 x 8: both gathers, the GEMM over the
    [splits][rows][chunk] slabs as a (1, kp) grid, the reduce"""
    from robustart_amd.model.train_engine import ResNet50TrainEngine, _TConv
    monkeypatch.setattr(_lib, 'require_gpu', lambda: torch)
    ready = []
    eng = _engine(ResNet50TrainEngine, monkeypatch, device=torch.device('cpu'), direct_wgrad=False, on_grad_ready=ready.append)
    conv = torch.nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False)
    conv.weight.grad = torch.zeros_like(conv.weight)
    tc = _TConv(conv, None, eng.device, torch)
    B, H, G = 2, 8, 4
    x, dz = _bf(B, H, H, 64), _bf(B, G, G, 64)
    kp = 9 * 64
    splits, chunk, n_rows = eb.wgrad_split_transposed(B * G * G, kp, 64)
    assert (splits, chunk, n_rows) == (1, 64, 64)
    eng._buf['wg_dzT'] = torch.ones(2 * n_rows * chunk * splits, dtype=torch.uint8)
    eng._conv_wgrad(tc, dz, (G, G), x, (H, H))
    (g_dz, g_x), (t_dz, t_x), d, red = _wgrad_calls(eng)
    dzt, colt, part = _check_wgrad_gemm(eng, d, kp, (1, kp), splits, chunk, n_rows, 64)
    assert g_dz == (dz.data_ptr(), dzt, B, G, G, 64, G, G, 1, 1, 1, splits * chunk, chunk, n_rows, None) and t_dz == ([0], [0])
    assert g_x == (x.data_ptr(), colt, B, H, H, 64, G, G, 2, 2, 9, splits * chunk, chunk, kp, None)
    assert list(zip(*t_x)) == tc.fwd_taps == [(r - 1, s - 1) for r in range(3) for s in range(3)]
    assert red == (part, splits, 9, 64, 64, 64, 64, conv.weight.grad.data_ptr(), 0, None)
    assert ready == [conv.weight]
    assert bool(eng._buf['wg_dzT'].all())                                # n_rows == n_pad: no tile-padding rows, nothing zeroed
    # the stem's form: 3 of the 4 channels of the padded plane kept by the reduce
    eng.lib.calls.clear()
    hi, dz1, w1 = _bf(B, 24, 24, 4), _bf(B, 8, 8, 64), torch.zeros(64, 3, 7, 7)
    taps = [(r, s) for r in range(7) for s in range(7)]
    eng._wgrad(dz1, 64, 64, hi, (24, 24), 4, (8, 8), taps, 2, w1, c_valid=3)
    (g_dz, g_x), (t_dz, t_x), d, red = _wgrad_calls(eng)
    assert g_x[2:11] == (B, 24, 24, 4, 8, 8, 2, 2, 49) and g_x[-2] == 196 and list(zip(*t_x)) == taps
    assert (d.grid_h, d.grid_w) == (1, 196) and red[1:7] == (1, 49, 3, 4, 64, 64)


def test_shared_weight_gradient_row_form(monkeypatch):
    """RowEngine._wgrad: 5 of the 6 rows of each of 2 images, 48 input features, 10 outputs in 64 columns; the GEMM as a (c_in, 1) grid"""
    monkeypatch.setattr(_lib, 'require_gpu', lambda: torch)
    eng = _engine(eb.RowEngine, monkeypatch, device=torch.device('cpu'))
    rows, c_in, n_out, n_pad = 2 * 5, 48, 10, 64
    dz, x, grad = _bf(2 * 6, n_pad), _bf(rows, c_in), torch.zeros(n_out, c_in)
    splits, chunk, n_rows = eb.wgrad_split_transposed(rows, c_in, n_pad)
    assert (splits, chunk, n_rows) == (1, 64, 64)
    eng._wgrad(dz, n_out, n_pad, x, c_in, grad, rows, dz_images=(2, 6, 5))
    (g_dz, g_x), (t_dz, t_x), d, red = _wgrad_calls(eng)
    dzt, colt, part = _check_wgrad_gemm(eng, d, c_in, (c_in, 1), splits, chunk, n_rows, 64)
    assert g_dz == (dz.data_ptr(), dzt, 2, 6, 1, n_pad, 5, 1, 1, 1, 1, splits * chunk, chunk, n_rows, None)
    assert g_x == (x.data_ptr(), colt, 1, rows, 1, c_in, rows, 1, 1, 1, 1, splits * chunk, chunk, c_in, None)
    assert t_dz == t_x == ([0], [0])
    assert red == (part, splits, 1, c_in, c_in, n_out, 64, grad.data_ptr(), 0, None)
    # without dz_images: one image of `rows` rows
    eng.lib.calls.clear()
    eng._wgrad(dz, n_out, n_pad, x, c_in, grad, rows)
    assert _wgrad_calls(eng)[0][0][2:8] == (1, rows, 1, n_pad, rows, 1)


def test_shared_weight_gradient_zeroes_the_tile_padding_rows_only_when_there_are_some(monkeypatch):
    """the transposed dz has n_rows = n_pad rounded up to the GEMM's column tile; rows n_pad .. n_rows are written by nobody, so the
    slabs are zeroed first when and only when n_rows > n_pad"""
    monkeypatch.setattr(_lib, 'require_gpu', lambda: torch)
    rows, c_in = 10, 48
    for n_pad, n_rows in ((64, 64), (128, 128), (40, 64), (200, 256), (72, 128)):
        eng = _engine(eb.RowEngine, monkeypatch, device=torch.device('cpu'))
        splits, chunk, got_rows = eb.wgrad_split_transposed(rows, c_in, n_pad)
        assert got_rows == n_rows
        used = n_rows * chunk * splits * 2
        buf = eng._buf['wg_dzT'] = torch.ones(used + 64, dtype=torch.uint8)
        eng._wgrad(_bf(rows, n_pad), n_pad, n_pad, _bf(rows, c_in), c_in, torch.zeros(n_pad, c_in), rows)
        assert eng._buf['wg_dzT'] is buf and bool(buf[used:].all())
        assert bool(buf[:used].all()) if n_rows == n_pad else not buf[:used].any()


def test_conv_tap_classes():
    """one geometry for the eval and the train engine: forward taps, filter taps, and per input-parity class of the backward to the
    input the (dy, dx) read from the output gradient and the filter taps that reach it"""
    for r, stride, pad in ((1, 1, 0), (3, 1, 1), (3, 2, 1), (1, 2, 0), (7, 2, 3)):
        fwd, all_rs, bwd = eb.conv_tap_classes(r, r, stride, pad)
        assert all_rs == [(a, b) for a in range(r) for b in range(r)]
        assert fwd == [(a - pad, b - pad) for a in range(r) for b in range(r)]
        if stride == 1:
            assert bwd == [(None, [(pad - a, pad - b) for a, b in all_rs], all_rs)]
            continue
        assert [p for p, _, _ in bwd] == [(0, 0), (0, 1), (1, 0), (1, 1)]
        for (ph, pw), taps, rs in bwd:
            assert rs == [(a, b) for a, b in all_rs if (ph + pad - a) % 2 == 0 and (pw + pad - b) % 2 == 0]
            assert taps == [((ph + pad - a) // 2, (pw + pad - b) // 2) for a, b in rs]
        assert sorted(t for _, _, rs in bwd for t in rs) == all_rs      # every filter tap reaches exactly one class
    assert [len(taps) for _, taps, _ in eb.conv_tap_classes(1, 1, 2, 0)[2]] == [1, 0, 0, 0]
    assert [len(taps) for _, taps, _ in eb.conv_tap_classes(3, 3, 2, 1)[2]] == [1, 2, 2, 4]
    assert [len(taps) for _, taps, _ in eb.conv_tap_classes(7, 7, 2, 3)[2]] == [9, 12, 12, 16]
    assert eb.conv_tap_classes(3, 3, 2, 1)[2][0] == ((0, 0), [(0, 0)], [(1, 1)])
    assert eb.conv_tap_classes(3, 3, 2, 1)[2][3][1] == [(1, 1), (1, 0), (0, 1), (0, 0)]


def test_both_resnet_engines_build_from_the_one_geometry():
    from robustart_amd.model.engine import _Conv
    from robustart_amd.model.train_engine import _TConv
    for cin, cout, r, stride in ((8, 16, 3, 1), (8, 16, 3, 2), (16, 8, 1, 2)):
        conv = torch.nn.Conv2d(cin, cout, r, stride=stride, padding=r // 2, bias=False)
        ev, tr = _Conv(conv, None, 'cpu'), _TConv(conv, None, torch.device('cpu'), torch)
        fwd, all_rs, classes = eb.conv_tap_classes(r, r, stride, r // 2)
        assert ev.fwd_taps == tr.fwd_taps == fwd and tr.all_rs == all_rs
        assert [(p, t) for p, t, _ in ev.bwd] == [(p, t) for p, t, _, _ in tr.bwd] == [(p, t) for p, t, _ in classes]
        assert [rs for _, _, rs, _ in tr.bwd] == [rs for _, _, rs in classes]
        for (_, taps, a), (_, _, _, b) in zip(ev.bwd, tr.bwd):
            assert (a is None and b is None and not taps) or a.shape == b.shape == (64, len(taps) * cout)
        assert ev.w_fwd.shape == tr.w_fwd.shape == (64, r * r * cin)
    w = torch.randn(64, 3, 7, 7)
    rows = eb.stem_rows(w).view(64, 7, 8, 4)
    assert torch.equal(rows[:, :, :7, :3], w.permute(0, 2, 3, 1)) and not rows[:, :, 7].any() and not rows[..., 3].any()


# ---------------------------------------------------------------------- the row engines against the recorded trace
def test_row_engines_launch_what_the_recorded_trace_says():
    """every launch (entry, scalars, descriptor fields, pointers by buffer / table name) and every weight table (shape, dtype, bytes)
    of the row engines and their train engines on tiny modules, in both precisions, equals tests/golden/row_engine_trace.json, which
    tests/golden/make_row_engine_trace.py recorded before these engines moved onto RowEngine's table builder and call path"""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    spec = importlib.util.spec_from_file_location('make_row_engine_trace', os.path.join(golden, 'make_row_engine_trace.py'))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    with open(os.path.join(golden, 'row_engine_trace.json')) as f:
        want = json.load(f)
    got = make.record()
    assert sorted(got) == sorted(want)
    for case in sorted(want):
        w, g = want[case], got[case]
        for i, (a, b) in enumerate(zip(w['launches'], g['launches'])):
            assert a == b, '%s: launch %d is %s, recorded %s' % (case, i, b, a)
        assert len(w['launches']) == len(g['launches']), case
        assert sorted(w['tables']) == sorted(g['tables']), case
        for name in sorted(w['tables']):
            assert w['tables'][name] == g['tables'][name], '%s: table %s' % (case, name)
