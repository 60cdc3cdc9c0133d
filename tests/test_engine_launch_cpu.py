"""The shared launch layer (robustart_amd/model/engine_base.py) without a GPU: descriptors built from CPU tensors, field by field,
through the builders and through the engines' adapters with the library call replaced by a recorder."""
import torch

from robustart_amd import _lib
from robustart_amd.model import engine_base as eb


class _Recorder:
    def __init__(self):
        self.descs = []

    def rart_conv_igemm_bf16(self, d, stream):
        self.descs.append(d._obj)
        return 0

    def rart_gemm_pair_bf16(self, d, stream):
        self.descs.append(d._obj)
        return 0


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
