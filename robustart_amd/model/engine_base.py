"""The host launch layer the HIP engines share: the flag tables of the two GEMM descriptors, one builder per descriptor, the weight-table
helpers, the tap geometry of a convolution, the split-K heuristics of the weight gradient, and `EngineBase` (device, buffers,
profiling, both weight-gradient paths) that every engine inherits.

The builders take tensors or None and only read `data_ptr()`, so they run on CPU tensors as well.  ResNet-50 keeps the adapter that
encodes its own convention, the conv form and [hi | lo | hi] weight tables (engine.py).  The row form of ViT-B/16, MLP-Mixer, ConvNeXt
and the ConvStem chain lives in `RowEngine`, once for both precisions:
  tables    `_f32` (fp32 copy on the device), `_table` (row table of a GEMM weight or of its transpose) and `_input_table` (the table
            of the GEMM that reads the image pair): the caller names the form, the builder picks the precision
  launches  `_mm` / `_input_gemm` / `_conv` (GEMM, image-pair GEMM, implicit-GEMM convolution), `_rows` (any row kernel whose
            rart_*_pair and rart_*_bf16 entries differ by hi / lo pointer pairs alone, activations marked with `act`), and the named
            irregular ones: `_avgpool`, `_pool_bwd`, `_patchify`, `_unpatchify`
  chain     `_image_dims`, `_head_logits`, `_forward_loss` (the prologue of every `forward_backward`)
`RowTrainMixin` is what the three train engines of these models share: model, `on_grad_ready`, `repack`, the kept forward."""
import ctypes

from .. import _lib

# rart_conv_desc flags (csrc/conv_igemm.hip)
F_RELU, F_OUT_F32, F_GELU, F_GELU_BWD = 1, 2, 4, 8
F_MASK_BITS = 16         # `mask` is a 1-bit tensor
F_PAIR = 32              # split-bf16 operands as 3 x the taps, lo planes of dst / res at dst_pair_off / res_pair_off
F_GELU_KEEP = 64         # dst = gelu(u), `mask` receives the pre-activation u (256 x 256 GEMM only)
F_MASK_RES = 128         # the 1-bit mask applies to the residual
# rart_gemm_pair_desc flags (csrc/rart_gemm_pair_dev.h); the epilogue flags have the values of their rart_conv_desc namesakes
GP_RELU, GP_OUT_F32, GP_GELU, GP_GELU_BWD, GP_W_INTERLEAVED, GP_GELU_KEEP = 1, 2, 4, 8, 16, 64

PRECISIONS = {'bf16': 'bf16', 'bf16x3': 'bf16x3', 'fp32x': 'bf16x3'}

ROW_TAPS = [((0, 0),) * n for n in range(33)]      # ROW_TAPS[n]: n taps at the row itself (row form, per-tap source offsets)


def check_precision(precision):
    """-> the engine's name of `precision` ('fp32x' is 'bf16x3')"""
    if precision not in PRECISIONS:
        raise ValueError('precision must be one of %s' % sorted(PRECISIONS))
    return PRECISIONS[precision]


def _addr(t):
    return None if t is None else t.data_ptr()


def cints(vals):
    return (ctypes.c_int * max(len(vals), 1))(*vals)


def lo_off(t):
    """element offset of the lo plane of a pair tensor [2][...]"""
    return (t[1].data_ptr() - t[0].data_ptr()) // 2


# ---------------------------------------------------------------------- weight tables
def rows_mult(n_cols):
    return 128 if n_cols > 64 else 64


def k32(n):
    """n rounded up to the 32-deep K step of the GEMMs"""
    return (n + 31) // 32 * 32


def pad_rows(w, mult):
    """[rows][K] -> contiguous [rows rounded up to mult][K], zero rows appended"""
    import torch
    r = (w.shape[0] + mult - 1) // mult * mult
    if r != w.shape[0]:
        w = torch.cat([w, torch.zeros(r - w.shape[0], w.shape[1], dtype=w.dtype, device=w.device)], 0)
    return w.contiguous()


def pad_k(w, k):
    """[rows][K] -> [rows][max(K, k)], zero columns appended"""
    import torch
    if k is not None and k > w.shape[1]:
        w = torch.cat([w, torch.zeros(w.shape[0], k - w.shape[1], dtype=w.dtype, device=w.device)], 1)
    return w


def split_hi_lo(t):
    """fp32 -> (hi, lo) bf16 with hi = bf16(t), lo = bf16(t - hi): the split-bf16 representation"""
    import torch
    hi = t.to(torch.bfloat16)
    return hi, (t - hi.float()).to(torch.bfloat16)


def pair(t):
    """fp32 tensor -> [2][...] bf16 planes (hi, lo)"""
    import torch
    return torch.stack(split_hi_lo(t)).contiguous()


def act(t):
    """marks an argument of `RowEngine._rows` as an activation: a bf16 tensor, in reference precision a pair [2][...] (None: null)"""
    return (t,)


def interleave_k32(hi, lo):
    """two bf16 planes [rows][K] -> [rows][2K]: per row and 32-deep K step the hi slice then the lo slice (GP_W_INTERLEAVED)"""
    import torch
    rows, k = hi.shape
    return torch.stack([hi.reshape(rows, k // 32, 32), lo.reshape(rows, k // 32, 32)], 2).reshape(rows, 2 * k).contiguous()


def stem_rows(w):
    """stem weights [64][3][7][7] -> the row-tap form [64][224]: one tap = one filter row, 8 px x 4 ch (zero at px 7 and ch 3)"""
    import torch
    t = torch.zeros(64, 7, 8, 4, dtype=w.dtype, device=w.device)
    t[:, :, :7, :3] = w.permute(0, 2, 3, 1)                              # [cout][r][s][c]
    return t.reshape(64, 7 * 32)


def conv_tap_classes(r, s, stride, pad):
    """the geometry of an r x s convolution of stride 1 or 2 -> (fwd_taps, all_rs, bwd).  fwd_taps: the (dy, dx) an output pixel reads per
    filter tap of all_rs = [(r, s)]; bwd: the classes of the backward to the input as [(parity, taps, rs)]: the (dy, dx) an input pixel
    reads from the output gradient and the filter taps rs that reach it.  Stride 1: one class, parity None; stride 2: one class per
    input parity (ph, pw), over the filter taps that reach it (none for some classes of a 1 x 1)"""
    all_rs = [(a, b) for a in range(r) for b in range(s)]
    fwd_taps = [(a - pad, b - pad) for a, b in all_rs]
    if stride == 1:
        return fwd_taps, all_rs, [(None, [(pad - a, pad - b) for a, b in all_rs], all_rs)]
    assert stride == 2
    bwd = []
    for ph in range(2):
        for pw in range(2):
            rs = [(a, b) for a, b in all_rs if (ph + pad - a) % 2 == 0 and (pw + pad - b) % 2 == 0]
            bwd.append(((ph, pw), [((ph + pad - a) // 2, (pw + pad - b) // 2) for a, b in rs], rs))
    return fwd_taps, all_rs, bwd


# ---------------------------------------------------------------------- descriptors
def conv_desc(src, wgt, dst, batch, grid, src_hw, src_pix, k_per_tap, taps, n_cols, dst_hw, dst_pix, bias=None, res=None, mask=None,
              sign_out=None, stats_out=None, flags=0, stride=(1, 1), dst_stride=(1, 1), dst_org=(0, 0), tap_src_off=None, batched=None,
              dst_pair_off=0, res_pair_off=0):
    """rart_conv_desc of one implicit GEMM: output pixel (b, y, x) of the batch x grid reads source pixel (y * sy + dy, x * sx + dx)
    (+ tap_src_off[t] elements) per tap (dy, dx) of `taps`, k_per_tap channels each, and writes n_cols channels at destination pixel
    (y * dst_sy + oy, x * dst_sx + ox).  batched = dict(n, inner, src=(outer, inner), wgt=(outer, inner), dst=(outer, inner)
    [, wgt_row_stride]): element strides of problem z = (z / inner, z % inner)."""
    d = _lib.ConvDesc()
    d.src, d.wgt, d.dst = src.data_ptr(), wgt.data_ptr(), dst.data_ptr()
    d.bias, d.res, d.mask, d.sign_out, d.bn_stats_out = _addr(bias), _addr(res), _addr(mask), _addr(sign_out), _addr(stats_out)
    d.batch, d.grid_h, d.grid_w = batch, grid[0], grid[1]
    d.src_h, d.src_w, d.src_pix_stride = src_hw[0], src_hw[1], src_pix
    d.k_per_tap, d.n_taps = k_per_tap, len(taps)
    d.sy, d.sx = stride
    for i, (dy, dx) in enumerate(taps):
        d.tap_dy[i], d.tap_dx[i] = dy, dx
        if tap_src_off:
            d.tap_src_off[i] = tap_src_off[i]
    d.n_cols = n_cols
    d.dst_h, d.dst_w = dst_hw
    d.dst_sy, d.dst_sx = dst_stride
    d.dst_oy, d.dst_ox = dst_org
    d.dst_pix_stride = dst_pix
    d.flags = flags
    d.dst_pair_off, d.res_pair_off = dst_pair_off, res_pair_off
    if batched:
        d.n_batched, d.z_inner = batched['n'], batched['inner']
        d.src_z_outer, d.src_z_inner = batched['src']
        d.wgt_z_outer, d.wgt_z_inner = batched['wgt']
        d.dst_z_outer, d.dst_z_inner = batched['dst']
        d.wgt_row_stride = batched.get('wgt_row_stride', 0)
    return d


def gemm_pair_desc(a, w, dst, N, lda, ldw, ldc, w_rows, M=0, K=0, bias=None, res=None, aux=None, mask_bits=None, sign_out=None, flags=0,
                   a_off=0, w_off=0, dst_off=0, w_lo_off=None, w_il=None, rows_per_image=0, src_rows_per_image=0, src_row_off=0,
                   dst_rows_per_image=0, dst_row_off=0, batched=None, batch=0, grid=None, src_hw=(0, 0), stride=(1, 1), k_per_tap=0,
                   taps=(), dst_hw=(0, 0), dst_stride=(1, 1), dst_org=(0, 0), tile=(0, 0), src2=None):
    """rart_gemm_pair_desc: (a_hi + a_lo)[M][K] . (w_hi + w_lo)[N][K]^T -> dst, three MFMA products per contraction.
    a / res / aux / dst: pair tensors [2][...] (dst with GP_OUT_F32: a plain fp32 tensor); *_off: element offsets inside a plane.
    w: a pair tensor, or with w_lo_off one table that holds the lo plane w_lo_off elements after the hi plane; w_il: the
    interleaved copy of w's planes (`interleave_k32`), which replaces them.  batched = dict(n, inner, a=(outer, inner),
    w=(outer, inner), c=(outer, inner)).  Row form unless `grid` is given; conv form: output pixel (b, y, x) of batch x grid reads
    source pixel (y * sy + dy, x * sx + dx) per tap (dy, dx), k_per_tap channels each (M and K follow from the geometry).
    src2 (conv form) = (pair tensor, its (h, w), (sy, sx), elements per pixel, k2): a second source read at pixel (y * sy, x * sx), whose k2
    channels follow the first source's K in the rows of w; the result is then a rart_gemm_pair2_desc (GemmPair2Desc) around the launch."""
    d2 = _lib.GemmPair2Desc() if src2 is not None else None
    d = d2.one if d2 is not None else _lib.GemmPairDesc()       # (d2.one is a view: filling it fills the two-source descriptor)
    if grid is not None:
        M, K = batch * grid[0] * grid[1], k_per_tap * len(taps) + (src2[4] if src2 is not None else 0)
    d.a_hi, d.a_lo = a[0].data_ptr() + 2 * a_off, a[1].data_ptr() + 2 * a_off
    if w_il is not None:
        d.w_hi, d.w_lo, ldw = w_il.data_ptr(), w_il.data_ptr() + 64, 2 * K
        flags |= GP_W_INTERLEAVED
    elif w_lo_off is not None:
        w_hi = w.data_ptr() + 2 * w_off
        d.w_hi, d.w_lo = w_hi, w_hi + 2 * w_lo_off
    else:
        d.w_hi, d.w_lo = w[0].data_ptr() + 2 * w_off, w[1].data_ptr() + 2 * w_off
    d.bias = _addr(bias)
    if res is not None:
        d.res_hi, d.res_lo = res[0].data_ptr() + 2 * dst_off, res[1].data_ptr() + 2 * dst_off
    if flags & GP_OUT_F32:
        d.dst_hi = dst.data_ptr() + 4 * dst_off
    else:
        d.dst_hi, d.dst_lo = dst[0].data_ptr() + 2 * dst_off, dst[1].data_ptr() + 2 * dst_off
    if aux is not None:
        d.aux_hi, d.aux_lo = aux[0].data_ptr() + 2 * dst_off, aux[1].data_ptr() + 2 * dst_off
    d.M, d.N, d.K, d.lda, d.ldw, d.ldc, d.w_rows = M, N, K, lda, ldw, ldc, w_rows
    d.rows_per_image, d.src_rows_per_image, d.src_row_off = rows_per_image, src_rows_per_image, src_row_off
    d.dst_rows_per_image, d.dst_row_off = dst_rows_per_image, dst_row_off
    d.flags = flags
    if batched:
        d.n_batched, d.z_inner = batched['n'], batched['inner']
        d.a_z_outer, d.a_z_inner = batched['a']
        d.w_z_outer, d.w_z_inner = batched['w']
        d.c_z_outer, d.c_z_inner = batched['c']
    if grid is not None:
        d.conv, d.batch, d.grid_h, d.grid_w = 1, batch, grid[0], grid[1]
        d.src_h, d.src_w, d.sy, d.sx = src_hw[0], src_hw[1], stride[0], stride[1]
        d.k_per_tap, d.n_taps = k_per_tap, len(taps)
        for i, (dy, dx) in enumerate(taps):
            d.tap_dy[i], d.tap_dx[i] = dy, dx
        d.dst_h, d.dst_w = dst_hw
        d.dst_sy, d.dst_sx = dst_stride
        d.dst_oy, d.dst_ox = dst_org
    d.mask_bits, d.sign_out = _addr(mask_bits), _addr(sign_out)
    d.tile_m, d.tile_n = tile
    if d2 is not None:
        a2, hw2, st2, lda2, k2 = src2
        d2.a2_hi, d2.a2_lo = a2[0].data_ptr(), a2[1].data_ptr()
        d2.lda2, d2.k2, d2.src2_h, d2.src2_w, d2.sy2, d2.sx2 = lda2, k2, hw2[0], hw2[1], st2[0], st2[1]
        return d2
    return d


def gemm_pair_cls_desc(a, w, dst, N, lda, ldw, ldc, w_rows, classes, **kw):
    """rart_gemm_pair_cls_desc: the conv-form launch `gemm_pair_desc(a, w, dst, ..., **kw)` would describe, as up to four classes in one grid.
    classes = [(taps, k_off, dst_org, src2)]: the (dy, dx) taps of the class, the first column of its slice in the rows of w, its
    destination origin and whether it also accumulates the second source kw['src2'] (class 0 only).  kw carries no taps / dst_org."""
    taps = [t for c in classes for t in c[0]]
    src2 = kw.pop('src2', None)
    one = gemm_pair_desc(a, w, dst, N, lda, ldw, ldc, w_rows, taps=taps, src2=src2, **kw)
    d = _lib.GemmPairClsDesc()
    ctypes.memmove(ctypes.byref(d.two), ctypes.byref(one), ctypes.sizeof(one))
    d.n_classes = len(classes)
    at = 0
    for i, (ctaps, k_off, org, s2) in enumerate(classes):
        c = d.cls[i]
        c.tap_begin, c.n_taps, c.k_off, c.dst_oy, c.dst_ox, c.src2 = at, len(ctaps), k_off, org[0], org[1], int(bool(s2))
        at += len(ctaps)
    return d


def tokmix_desc(a, x, dst, M, N, K, batch, x_stride, c_stride, ldx=None, ldc=None, bias=None, res=None, aux=None, flags=0, pair=False):
    """rart_tokmix_desc of MLP-Mixer's token-mixing GEMM: C_b[m][n] = sum_k A[m][k] X_b[k][n] for images b < batch.  a: the weight table
    [M][lda] (K padded with zero columns; a pair [2][M][lda] when `pair`); x / dst / res / aux: per-image slabs x_stride / c_stride
    elements apart (pairs [2][...] when `pair`, dst a plain fp32 tensor with GP_OUT_F32); ldx / ldc default to N."""
    d = _lib.TokmixDesc()
    if pair:
        d.a_hi, d.a_lo, d.x_hi, d.x_lo = a[0].data_ptr(), a[1].data_ptr(), x[0].data_ptr(), x[1].data_ptr()
        if flags & GP_OUT_F32:
            d.dst_hi = dst.data_ptr()
        else:
            d.dst_hi, d.dst_lo = dst[0].data_ptr(), dst[1].data_ptr()
        if res is not None:
            d.res_hi, d.res_lo = res[0].data_ptr(), res[1].data_ptr()
        if aux is not None:
            d.aux_hi, d.aux_lo = aux[0].data_ptr(), aux[1].data_ptr()
    else:
        d.a_hi, d.x_hi, d.dst_hi, d.res_hi, d.aux_hi = a.data_ptr(), x.data_ptr(), dst.data_ptr(), _addr(res), _addr(aux)
    d.bias = _addr(bias)
    d.M, d.N, d.K, d.lda = M, N, K, a.shape[-1]
    d.ldx, d.ldc = ldx or N, ldc or N
    d.batch, d.flags = batch, flags
    d.x_stride, d.c_stride = x_stride, c_stride
    return d


def tokmix_wgrad_desc(p, q, partial, M, N, D, batch, splits, images_per_split, ld_partial, p_stride=None, q_stride=None):
    """rart_tokmix_wgrad_desc of a token-mixing weight gradient: partial[z][n][m] = sum over split z's images b and channels d of
    p_b[m][d] q_b[n][d].  p / q: bf16 per-image slabs [batch][M][D] / [batch][N][D], p_stride / q_stride elements apart (default:
    dense); partial: fp32 [splits][N][ld_partial]."""
    d = _lib.TokmixWgradDesc()
    d.p, d.q, d.partial = p.data_ptr(), q.data_ptr(), partial.data_ptr()
    d.M, d.N, d.D, d.batch = M, N, D, batch
    d.splits, d.images_per_split, d.ld_partial = splits, images_per_split, ld_partial
    d.p_stride, d.q_stride = p_stride or M * D, q_stride or N * D
    return d


# ---------------------------------------------------------------------- split-K weight gradients
def wgrad_split_direct(M, x_c, n_taps, n_cols, target_wgs, min_chunk):
    """-> (splits, chunk) of rart_wgrad_direct_bf16 over M output positions: about target_wgs workgroups in all, chunks of at least
    min_chunk positions"""
    tmr = 128                # the library's tile height (csrc/wgrad_direct.hip: 256-row tiles measured slower)
    if x_c == 4:             # the ResNet stem's padded hi plane: 32 taps x 4 channels per tile
        row_tiles = (n_taps + 31) // 32
    else:
        row_tiles = n_taps * (x_c // tmr) if x_c >= tmr else (n_taps + tmr // x_c - 1) // (tmr // x_c)
    tiles = row_tiles * (n_cols // (128 if n_cols % 128 == 0 else 64))
    splits = max(1, min(target_wgs // max(tiles, 1), M // min_chunk if M >= 2 * min_chunk else 1, 1024))
    chunk = ((M + splits - 1) // splits + 31) // 32 * 32
    return (M + chunk - 1) // chunk, chunk


def wgrad_split_transposed(M, kp, n_pad):
    """-> (splits, chunk, n_rows) of the split-K weight-gradient GEMM over transposed copies ([splits][rows][chunk] slabs): kp rows
    of the transposed im2col, n_pad gradient columns padded to the GEMM's n_rows"""
    bn_tile = 128 if n_pad > 64 else 64
    tiles = ((kp + 127) // 128) * ((n_pad + bn_tile - 1) // bn_tile)
    splits = max(1, min(1024 // max(tiles, 1), M // 512 if M >= 1024 else 1, 256))
    chunk = ((M + splits - 1) // splits + 63) // 64 * 64
    return splits, chunk, (n_pad + bn_tile - 1) // bn_tile * bn_tile


def wgrad_split_tokens(batch, M, N, target_wgs):
    """-> (splits, images_per_split) of rart_tokmix_wgrad_bf16: its contraction runs over images and channels, so it is split over
    whole images: split z sums images [z * images_per_split, min(batch, (z + 1) * images_per_split)), about target_wgs workgroups
    (128 x 128 output tiles x splits) in all, never more splits than images and no empty split"""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    splits = max(1, min(batch, target_wgs // tiles))
    per = (batch + splits - 1) // splits
    return (batch + per - 1) // per, per


# ---------------------------------------------------------------------- engines
class EngineBase:
    """Device, library, precision, name-keyed buffers and launch profiling of a HIP engine."""
    # K splits of rart_wgrad_direct_bf16: ~1 024 workgroups in all (measured at B = 256 on ResNet-50: 512 -> 58.1, 1 024 -> 55.1-55.8,
    # 2 048 -> 56.3, 4 096 -> 57.5 ms per adv_train step: more splits fill the CUs, every split writes and re-reads an fp32 copy of the
    # weight tensor); up to 1 024 splits of >= 256 positions each (a cap of 256 left layer1's one- and two-tile 1x1 layers at 256-512
    # workgroups: +0.6 ms)
    wgrad_target_wgs, wgrad_min_chunk = 1024, 256

    def __init__(self, device='cuda', precision='bf16'):
        torch = _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.precision = check_precision(precision)
        self.profile = None      # set to a list to record (flops, start_event, end_event, kind[, algorithmic bytes]) per launch
        self._buf = {}
        self._w_il = {}          # interleaved copies of pair weight tables (GP_W_INTERLEAVED), keyed by the table's address

    @property
    def x3(self):
        """reference precision: every activation, gradient and weight a hi + lo pair of bf16 planes"""
        return self.precision == 'bf16x3'

    def _get(self, name, shape, dtype=None, zero=False):
        torch = _lib.require_gpu()
        dtype = dtype or torch.bfloat16
        t = self._buf.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
            self._buf[name] = t
        return t

    def _scratch(self, name, nbytes):
        torch = _lib.require_gpu()
        t = self._buf.get(name)
        if t is None or t.numel() < nbytes:
            t = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            self._buf[name] = t
        return t

    # precision-generic helpers: a bf16 tensor or a pair [2][...], the bf16 or the pair library entry
    def _act(self, name, shape):
        """activation buffer: bf16 [shape], or the pair [2][shape]"""
        return self._get(name, ((2,) + tuple(shape)) if self.x3 else tuple(shape))

    def _hl(self, t):
        return (_lib.ptr(t[0]), _lib.ptr(t[1])) if self.x3 else (_lib.ptr(t), None)

    def _dlogits_rows(self, dl, name, B, kpad):
        """-> the fp32 loss gradient dl [B][n_classes] as rows of kpad columns (zero past n_classes) in the engine's precision"""
        lib, sp = self.lib, _lib.stream_ptr()
        dlb = self._act(name, (B, kpad))
        if self.x3:
            _lib.check(lib.rart_f32_to_pair_rows(_lib.ptr(dl), _lib.ptr(dlb[0]), lo_off(dlb), B, self.n_classes, kpad, sp))
        else:
            _lib.check(lib.rart_f32_to_bf16_rows(_lib.ptr(dl), _lib.ptr(dlb), B, self.n_classes, kpad, sp))
        return dlb

    def _prof_begin(self):
        if self.profile is None:
            return None
        e0 = _lib.require_gpu().cuda.Event(enable_timing=True)
        e0.record()          # torch's current stream == the stream the kernel is enqueued on (stream_ptr())
        return e0

    def _prof_end(self, e0, flops, kind, nbytes=None):
        e1 = _lib.require_gpu().cuda.Event(enable_timing=True)
        e1.record()
        self.profile.append((flops, e0, e1, kind) if nbytes is None else (flops, e0, e1, kind, nbytes))

    def _launch_conv(self, d):
        """rart_conv_igemm_bf16 on descriptor d; profiled as 'igemm' (FLOPs of the listed taps)"""
        ev = self._prof_begin()
        _lib.check(self.lib.rart_conv_igemm_bf16(ctypes.byref(d), _lib.stream_ptr()))
        if ev is not None:
            self._prof_end(ev, 2.0 * d.batch * d.grid_h * d.grid_w * d.k_per_tap * d.n_taps * d.n_cols * max(d.n_batched, 1), 'igemm')

    def _launch_pair(self, d, nbytes=None):
        """rart_gemm_pair_bf16 on descriptor d (rart_gemm_pair2_bf16 on a two-source descriptor); profiled as 'gemm_pair' (MFMA FLOPs
        issued: three products; K of a two-source launch counts both sources)"""
        ev = self._prof_begin()
        if isinstance(d, _lib.GemmPair2Desc):
            _lib.check(self.lib.rart_gemm_pair2_bf16(ctypes.byref(d), _lib.stream_ptr()))
            d = d.one
        else:
            _lib.check(self.lib.rart_gemm_pair_bf16(ctypes.byref(d), _lib.stream_ptr()))
        if ev is not None:
            self._prof_end(ev, 3 * 2.0 * max(d.n_batched, 1) * d.M * d.N * d.K, 'gemm_pair', nbytes)

    def _launch_pair_classes(self, d, nbytes=None):
        """rart_gemm_pair_classes_bf16 on descriptor d; profiled as 'gemm_pair' (MFMA FLOPs issued over all classes)"""
        ev = self._prof_begin()
        _lib.check(self.lib.rart_gemm_pair_classes_bf16(ctypes.byref(d), _lib.stream_ptr()))
        if ev is not None:
            one = d.two.one
            k = sum(one.k_per_tap * d.cls[i].n_taps + (d.two.k2 if d.cls[i].src2 else 0) for i in range(d.n_classes))
            self._prof_end(ev, 3 * 2.0 * one.M * one.N * k, 'gemm_pair', nbytes)

    def _launch_tokmix(self, d, pair):
        """rart_tokmix_{bf16,pair} on descriptor d; profiled as 'tokmix' (MFMA FLOPs issued: three products in pair form)"""
        ev = self._prof_begin()
        _lib.check((self.lib.rart_tokmix_pair if pair else self.lib.rart_tokmix_bf16)(ctypes.byref(d), _lib.stream_ptr()))
        if ev is not None:
            self._prof_end(ev, (3 if pair else 1) * 2.0 * d.batch * d.M * d.N * d.K, 'tokmix')

    def _wgrad_direct(self, x, dz, B, x_hw, x_c, grid_hw, n_out, n_pad_cols, taps, stride, grad, c_valid=None):
        """grad[n_out][c][taps] = sum over positions m of dz[m][n] * x[pixel(m) + tap][c] straight from the NHWC activations
        (x: bf16 [B][ih][iw][x_c], dz: bf16 [B][gh][gw][n_pad_cols], columns >= n_out zero; c_valid: channels of x kept) on
        rart_wgrad_direct_bf16 + rart_wgrad_reduce_f32"""
        lib, sp = self.lib, _lib.stream_ptr()
        splits, chunk = wgrad_split_direct(B * grid_hw[0] * grid_hw[1], x_c, len(taps), n_pad_cols, self.wgrad_target_wgs,
                                           self.wgrad_min_chunk)
        part = self._scratch('wg_part', splits * len(taps) * x_c * n_pad_cols * 4)
        _lib.check(lib.rart_wgrad_direct_bf16(_lib.ptr(x), _lib.ptr(dz), _lib.ptr(part), B, x_hw[0], x_hw[1], x_c, grid_hw[0], grid_hw[1],
                                              n_pad_cols, stride, stride, len(taps), cints([t[0] for t in taps]), cints([t[1] for t in taps]),
                                              splits, chunk, n_pad_cols, sp))
        _lib.check(lib.rart_wgrad_reduce_f32(_lib.ptr(part), splits, len(taps), c_valid if c_valid is not None else x_c, x_c, n_out,
                                             n_pad_cols, _lib.ptr(grad), 0, sp))

    def _wgrad_transposed(self, dz, dz_geom, x, x_geom, n_out, grad, reduce, row_grid=False):
        """grad[n_out][c][taps] = sum_m dz[m][n] * x[pixel(m) + tap][c] as a split-K GEMM on the igemm kernel over transposed copies
        of both operands, one compact slab per K split: [splits][rows][chunk].  dz_geom = (images, src_h, src_w, channels, grid_h,
        grid_w): position m is pixel (y, x) of the grid_h x grid_w grid of an image of src_h x src_w pixels, `channels` bf16 values
        each (columns >= n_out zero); x_geom: the same for x, then (stride, taps): the pixel a position reads per tap.  reduce =
        (n_taps, c_valid, x_c) of rart_wgrad_reduce_f32.  row_grid: the GEMM's rows as a (rows, 1) grid, the row form's
        descriptor, instead of (1, rows): the 256 x 256 kernel's eligibility test reads the grid's width."""
        lib, sp = self.lib, _lib.stream_ptr()
        n_pad = dz_geom[3]
        images, x_h, x_w, x_c, grid_h, grid_w, stride, taps = x_geom
        kp = len(taps) * x_c                                   # rows of the transposed im2col matrix
        splits, chunk, n_rows = wgrad_split_transposed(images * grid_h * grid_w, kp, n_pad)
        m_pad = chunk * splits
        dzt = self._scratch('wg_dzT', n_rows * m_pad * 2)
        colt = self._scratch('wg_colT', kp * m_pad * 2)
        zero = cints([0])
        if n_rows > n_pad:
            dzt[:n_rows * m_pad * 2].zero_()                     # tile-padding rows of every slab stay zero
        _lib.check(lib.rart_transpose_gather_bf16(_lib.ptr(dz), _lib.ptr(dzt), *dz_geom, 1, 1, 1, zero, zero, m_pad, chunk, n_rows, sp))
        _lib.check(lib.rart_transpose_gather_bf16(_lib.ptr(x), _lib.ptr(colt), images, x_h, x_w, x_c, grid_h, grid_w, stride, stride,
                                                  len(taps), cints([t[0] for t in taps]), cints([t[1] for t in taps]), m_pad, chunk,
                                                  kp, sp))
        ld_n = (n_pad + 7) // 8 * 8
        part = self._scratch('wg_part', splits * kp * ld_n * 4)
        grid = (kp, 1) if row_grid else (1, kp)
        self._launch_conv(conv_desc(colt, dzt, part, 1, grid, grid, chunk, chunk, ROW_TAPS[1], ld_n, grid, ld_n, flags=F_OUT_F32,
                                    batched=dict(n=splits, inner=splits, src=(0, kp * chunk), wgt=(0, n_rows * chunk), dst=(0, kp * ld_n),
                                                 wgt_row_stride=chunk)))
        _lib.check(lib.rart_wgrad_reduce_f32(_lib.ptr(part), splits, *reduce, n_out, ld_n, _lib.ptr(grad), 0, sp))

    def _colsum(self, x, ld, rows, cols, out):
        lib = self.lib
        need = lib.rart_colsum_workspace_bytes(rows, cols)
        ws = self._scratch('cs_ws', need)
        _lib.check(lib.rart_colsum_bf16(_lib.ptr(x), ld, rows, cols, _lib.ptr(out), 0, _lib.ptr(ws), need, _lib.stream_ptr()))

    def logits(self, x01, mean, std):
        """x01: fp32 NCHW in [0,1]; mean/std: 3-tuples applied inside the input kernel."""
        return self._logits(x01.detach().float().contiguous(), False, mean, std)

    def logits_from_u8(self, batch_u8, mean, std):
        """batch_u8: uint8 NHWC (the corruption kernels' output) -> logits, normalisation fused."""
        return self._logits(batch_u8, True, mean, std)

    def _logits(self, src, src_is_u8, mean, std):
        """the inference forward: nothing kept for a backward (ResNet-50's `_forward` also returns its activations)"""
        return self._forward(src, src_is_u8, mean, std)


class RowEngine(EngineBase):
    """The row form of ViT-B/16, MLP-Mixer and ConvNeXt: activations are dense [rows][features] matrices (tokens, NHWC pixels).
    `_gemm` / `_gemm_pair` are the two GEMM launchers; the table builders before them and the helpers after them take either
    precision: a bf16 tensor or a pair [2][...], the bf16 or the pair library entry."""

    # ------------------------------------------------------------------ weight tables, in the engine's precision
    def _f32(self, t):
        """fp32 copy of a parameter on the engine's device"""
        import torch
        return t.detach().to(self.device, torch.float32).contiguous()

    def _table(self, w2d, k_pad=None, transpose=False, interleave=False):
        """row table of the GEMM weight w2d [rows][K], or with `transpose` of W^T (the backward-to-input table), K zero-padded to
        k_pad: pair planes [2][rows padded to the 256-row tile of rart_gemm_pair_bf16][K] in reference precision, else bf16 with rows
        padded to rows_mult(rows).  Padding rows are zero and never stored.  interleave (pair planes with K a multiple of 32): keep
        their interleaved copy beside them in `_w_il`, keyed by their address (GP_W_INTERLEAVED: one 128-byte line per row and K step)"""
        import torch
        w = w2d.detach().to(self.device, torch.float32)
        if self.x3:
            t = pair(pad_rows(pad_k(w.t() if transpose else w, k_pad), 256))
            if interleave and t.shape[2] % 32 == 0:
                self._w_il[t.data_ptr()] = interleave_k32(t[0], t[1])
            return t
        w = w.to(torch.bfloat16)
        t = pad_k(w.t() if transpose else w, k_pad)
        return pad_rows(t, rows_mult(t.shape[0]))

    def _input_table(self, w2d, rows_mult, interleave=False):
        """table of the GEMM that reads the image pair (`_input_gemm`): the pair table in reference precision, else bf16 [hi | hi]
        columns, which the hi and the lo plane of the image meet as two taps, rows padded to a multiple of `rows_mult`"""
        if self.x3:
            return self._table(w2d, interleave=interleave)
        import torch
        w = w2d.detach().to(self.device, torch.float32).to(torch.bfloat16)
        return pad_rows(torch.cat([w, w], 1), rows_mult)

    def _gemm(self, src, wgt, dst, rows, k, n_cols, src_ld, dst_ld, bias=None, res=None, flags=0, n_taps=1,
              tap_src_off=None, rows_per_image=None, dst_rows_per_image=None, dst_row_off=0, batched=None,
              src_rows_per_image=None, mask=None):
        """rows x k (x n_taps) times wgt^T -> dst on rart_conv_igemm_bf16.  rows_per_image/dst_rows_per_image/dst_row_off place the
        output rows of image b at b*dst_rows_per_image + dst_row_off (class-token slot).  batched: as `conv_desc`'s."""
        rpi = rows_per_image or rows
        self._launch_conv(conv_desc(src, wgt, dst, rows // rpi, (rpi, 1), (src_rows_per_image or rpi, 1), src_ld, k, ROW_TAPS[n_taps],
                                    n_cols, (dst_rows_per_image or rpi, 1), dst_ld, bias=bias, res=res, mask=mask, flags=flags,
                                    dst_org=(dst_row_off, 0), tap_src_off=tap_src_off, batched=batched))

    def _gemm_pair(self, a, w, dst, M, N, K, lda, ldc, ldw=None, bias=None, res=None, flags=0, aux=None, w_rows=None,
                   rows_per_image=0, src_rows_per_image=0, src_row_off=0, dst_rows_per_image=0, dst_row_off=0, batched=None,
                   a_off=0, w_off=0, dst_off=0):
        """(a_hi + a_lo)[M][K] . (w_hi + w_lo)[N][K]^T -> dst on rart_gemm_pair_bf16 (see `gemm_pair_desc`); w: pair planes
        [2][rows][K], replaced by their interleaved copy in `_w_il` when there is one."""
        il = self._w_il.get(w.data_ptr()) if (w_off == 0 and ldw is None and not batched) else None
        self._launch_pair(gemm_pair_desc(a, w, dst, N, lda, ldw or K, ldc, w_rows if w_rows is not None else w.shape[-2], M=M, K=K,
                                         bias=bias, res=res, aux=aux, flags=flags, a_off=a_off, w_off=w_off, dst_off=dst_off,
                                         w_il=il if il is not None and il.shape[1] == 2 * K else None, rows_per_image=rows_per_image,
                                         src_rows_per_image=src_rows_per_image, src_row_off=src_row_off,
                                         dst_rows_per_image=dst_rows_per_image, dst_row_off=dst_row_off, batched=batched))

    # ------------------------------------------------------------------ precision-generic launches
    def _mm(self, a, w, dst, M, N, K, lda=None, ldc=None, aux=None, src_row_off=0, **kw):
        """dst[M][N] = a[M][K] . w[N][K]^T; kw: bias, res, flags (the F_* values, which the GP_* flags share; aux = the GELU
        pre-activation kept / read) and rows_per_image, src_rows_per_image, dst_rows_per_image, dst_row_off: image b's rows are
        src_rows_per_image * b + src_row_off + (0 .. rows_per_image) of a and dst_rows_per_image * b + dst_row_off + ... of dst."""
        lda, ldc = lda or K, ldc or N
        if self.x3:
            self._gemm_pair(a, w, dst, M, N, K, lda, ldc, aux=aux, src_row_off=src_row_off, **kw)
        else:       # rart_conv_desc has no source row offset: start at that row
            self._gemm(a.view(-1, lda)[src_row_off:] if src_row_off else a, w, dst, M, K, N, lda, ldc, mask=aux, **kw)

    def _input_gemm(self, patches, w, dst, rows, N, K, ldc=None, **kw):
        """dst[rows][N] = patches . w^T for the image pair `patches` [2][rows][K] and its `_input_table`: the pair GEMM, or in bf16
        the hi and the lo plane as two taps of the [hi | hi] columns; kw: as `_mm`'s"""
        if self.x3:
            self._gemm_pair(patches, w, dst, rows, N, K, K, ldc or N, **kw)
        else:
            self._gemm(patches[0], w, dst, rows, K, N, K, ldc or N, n_taps=2, tap_src_off=[0, lo_off(patches)], **kw)

    def _conv(self, src, w, dst, B, grid, src_hw, src_ld, taps, n_cols, dst_hw, dst_ld, stride, dst_stride, dst_org, bias=None):
        """implicit-GEMM convolution on NHWC src (rows src_ld apart, all of them contracted) -> n_cols channels of dst (rows dst_ld apart)"""
        if self.x3:
            self._launch_pair(gemm_pair_desc(src, w, dst, n_cols, src_ld, src_ld * len(taps), dst_ld, w.shape[1], bias=bias, batch=B,
                                             grid=grid, src_hw=src_hw, stride=stride, k_per_tap=src_ld, taps=taps, dst_hw=dst_hw,
                                             dst_stride=dst_stride, dst_org=dst_org))
        else:
            self._launch_conv(conv_desc(src, w, dst, B, grid, src_hw, src_ld, src_ld, taps, n_cols, dst_hw, dst_ld, bias=bias,
                                        stride=stride, dst_stride=dst_stride, dst_org=dst_org))

    def _rows(self, stem, *args):
        """one launch of the row kernel rart_<stem>_pair / rart_<stem>_bf16, entries that differ by hi / lo pointer pairs alone.
        args in the entry's order: `act(t)` for an activation (hi and lo pointer in reference precision, one pointer in bf16), any
        other tensor (fp32 parameters, statistics) as it is, scalars as they are; the stream is appended"""
        x3, a = self.x3, []
        for v in args:
            if isinstance(v, tuple):             # act(t)
                t, = v
                a += [_lib.ptr(p) for p in ((t,) if not x3 else (None, None) if t is None else (t[0], t[1]))]
            else:
                a.append(_lib.ptr(v) if hasattr(v, 'data_ptr') else v)
        _lib.check(getattr(self.lib, 'rart_%s_%s' % (stem, 'pair' if x3 else 'bf16'))(*a, _lib.stream_ptr()))

    def _ln(self, x, g, b, out, rows, c, ld_in=None, ld_out=None):
        """out = LayerNorm(x) over the c features of `rows` rows ld_in / ld_out elements apart (default: dense)"""
        self._rows('layernorm', act(x), g, b, act(out), rows, c, ld_in or c, ld_out or c, 1e-6)

    def _ln_bwd(self, dy, x, g, res, dx, rows, c, strides=None):
        """dx = LayerNorm'(x)^T dy (+ res); strides: the row strides of (dy, x, res, dx), default dense"""
        ld = strides or (c, c, c if res is not None else 0, c)
        self._rows('layernorm_bwd', act(dy), act(x), g, act(res), act(dx), rows, c, *ld, 1e-6)

    def _avgpool(self, x, out, B, P, C):
        """out[B][C] = the mean over the P rows of every image of x [B][P][C]"""
        lib, sp = self.lib, _lib.stream_ptr()
        if self.x3:          # the pair entry takes the hi pointers and the plane sizes
            _lib.check(lib.rart_engine_avgpool_pair(_lib.ptr(x[0]), x[0].numel(), _lib.ptr(out[0]), out[0].numel(), B, P, C, sp))
        else:
            _lib.check(lib.rart_engine_avgpool(_lib.ptr(x), _lib.ptr(out), B, P, C, sp))

    def _pool_bwd(self, dpooled, dx, B, P, C):
        """the backward of `_avgpool`: dx[B][P][C] = dpooled[B][C] / P at every row"""
        self._rows('cnx_pool_bwd', act(dpooled), act(dx), B, P, C)

    def _fc1_gelu(self, ln, w, b, hid, u, rows, K, N, keep):
        """hid = gelu(ln . w^T + b), the fc1 of a transformer MLP; keep: u receives the pre-activation (GELU' in the backward)"""
        if not keep:
            self._mm(ln, w, hid, rows, N, K, bias=b, flags=F_GELU)
        elif self.x3 or self.lib.rart_gemm256_supported(rows, K, N, K, N):
            self._mm(ln, w, hid, rows, N, K, bias=b, flags=F_GELU_KEEP, aux=u)       # one launch writes both
        else:                        # bf16: only the 256 x 256 GEMM keeps the pre-activation
            self._mm(ln, w, u, rows, N, K, bias=b)
            _lib.check(self.lib.rart_gelu_bf16(_lib.ptr(u), _lib.ptr(hid), u.numel(), _lib.stream_ptr()))

    def _patchify(self, src, src_is_u8, mean, std, B, H, W, ps):
        """-> the normalised ps x ps patches of the image batch as the pair [2][B][patches][3 * ps * ps] (in both precisions)"""
        patches = self._get('patches', (2, B, (H // ps) * (W // ps), 3 * ps * ps))
        meanf, stdf = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        _lib.check(self.lib.rart_vit_patchify(_lib.ptr(src), 1 if src_is_u8 else 0, _lib.ptr(patches[0]), _lib.ptr(patches[1]),
                                              B, H, W, ps, meanf, stdf, _lib.stream_ptr()))
        return patches

    def _unpatchify(self, dpatch, B, H, W, ps, std, ld=None):
        """-> d(loss)/d(x01) fp32 NCHW from the patch gradient [B * patches][ld] (default 3 * ps * ps columns), bf16 or fp32"""
        torch = _lib.require_gpu()
        grad = torch.empty(B, 3, H, W, dtype=torch.float32, device=self.device)
        fn = self.lib.rart_vit_unpatchify_from_f32 if dpatch.dtype == torch.float32 else self.lib.rart_vit_unpatchify_f32
        _lib.check(fn(_lib.ptr(dpatch), _lib.ptr(grad), B, H, W, ps, ld or 3 * ps * ps, (ctypes.c_float * 3)(*std), _lib.stream_ptr()))
        return grad

    # ------------------------------------------------------------------ the ends of every chain
    @staticmethod
    def _image_dims(src, src_is_u8):
        """-> (B, H, W) of an image batch, u8 NHWC or fp32 NCHW"""
        return (src.shape[0], src.shape[1], src.shape[2]) if src_is_u8 else (src.shape[0], src.shape[2], src.shape[3])

    def _head_logits(self, feat, B, K):
        """-> the fp32 logits [B][n_classes] = feat[B][K] . head_w^T + head_b"""
        torch = _lib.require_gpu()
        logits = torch.empty(B, self.n_classes, dtype=torch.float32, device=self.device)
        self._mm(feat, self.head_w, logits, B, self.n_classes, K, bias=self.head_b, flags=F_OUT_F32)
        return logits

    def _forward_loss(self, x01, mean, std, y, kind, y_target, scale, name, K):
        """the prologue of every `forward_backward`: the forward that keeps its activations in `_saved`, the loss, and the head's dgrad
        GEMM -> (logits, loss, pred, the gradient [B][K] of the head's input in buffer `name`)"""
        from ..noise.adv import logit_loss
        logits = self._forward(x01.detach().float().contiguous(), False, mean, std, keep=True)
        loss, dl, pred = logit_loss(logits, y, kind, y_target, scale)
        self.last_dlogits = dl           # exposed for the parity tests (same upstream gradient for the reference)
        B, kp = logits.shape[0], self.head_kpad
        dfeat = self._act(name, (B, K))
        self._mm(self._dlogits_rows(dl, 'g_dl', B, kp), self.head_wd, dfeat, B, K, kp)
        return logits, loss, pred, dfeat

    # train engines (`RowTrainMixin`): they set `on_grad_ready`, called once per parameter after the last kernel that writes or reads
    # its gradient has been enqueued
    def _ln_bwd_full(self, dy, x, gamma, res, dx, rows, c, norm, strides=None):
        """the backward of `_ln_bwd` plus the gradients of `norm`'s weight and bias (bf16)"""
        lib = self.lib
        ld = strides or (c, c, c if res is not None else 0, c)
        need = lib.rart_layernorm_bwd_workspace_bytes(c)
        ws = self._scratch('ln_ws', need)
        _lib.check(lib.rart_layernorm_bwd_full_bf16(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(gamma), _lib.ptr(res), _lib.ptr(dx), rows,
                                                    c, *ld, 1e-6, _lib.ptr(norm.weight.grad), _lib.ptr(norm.bias.grad), 0,
                                                    _lib.ptr(ws), need, _lib.stream_ptr()))
        self.on_grad_ready(norm.weight)
        self.on_grad_ready(norm.bias)

    def _linear_grads(self, lin, dz, n_pad, x, rows, dz_images=None):
        """the weight gradient of the Linear (or patch convolution) `lin` from its output gradient dz and its input x, see `_wgrad`"""
        n_out, c_in = lin.weight.shape[0], lin.weight[0].numel()
        self._wgrad(dz, n_out, n_pad, x, c_in, lin.weight.grad, rows, dz_images)
        self.on_grad_ready(lin.weight)

    def _wgrad(self, dz, n_out, n_pad, x, c_in, grad, rows, dz_images=None):
        """grad[n_out][c_in] = dz^T . x (dz: bf16 [rows][n_pad] dense, columns >= n_out zero; x: bf16 [rows][c_in] dense) as a split-K
        GEMM over transposed copies (`_wgrad_transposed`).  dz_images = (B, rows_per_image_in_memory, rows_used): dz rows are the first
        `rows_used` of every image block."""
        b, sh, gh = dz_images if dz_images is not None else (1, rows, rows)
        self._wgrad_transposed(dz, (b, sh, 1, n_pad, gh, 1), x, (1, rows, 1, c_in, rows, 1, 1, ROW_TAPS[1]), n_out, grad,
                               (1, c_in, c_in), row_grid=True)


class RowTrainMixin:
    """What the train engines of the row models share, mixed in before the evaluation engine they extend (bf16): the module whose
    `.grad` tensors `backward` fills, `on_grad_ready(param)`, `repack` and the forward that keeps its activations."""

    def __init__(self, model, device='cuda', on_grad_ready=None):
        super().__init__(model, device)
        self.model = model
        self.on_grad_ready = on_grad_ready or (lambda p: None)

    def repack(self):
        """fp32 master weights -> bf16 tables; call after every optimizer step."""
        self.refold(self.model)

    def forward(self, src, src_is_u8, mean, std):
        if not src_is_u8:
            src = src.detach().float().contiguous()
        return self._forward(src, src_is_u8, mean, std, keep=True)
