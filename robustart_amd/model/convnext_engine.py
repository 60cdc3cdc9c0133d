"""ConvNeXt-B and ConvNeXt-V2-B forward and backward-to-input on the hand-written HIP kernels (evaluation of clean / corrupted images;
the gradient step of every attack, adv/attack.py:21-22, autopgd_base.py:271-289).  Reference module: robustart_amd/model/convnext_torch.py.

Layout: NHWC activations, rows = (image, y, x).  Per launch:
  stem        rart_cnx_patchify (4x4 patches, K = 48 padded to 64, hi + lo planes) -> GEMM (+ bias) -> LayerNorm
              (`convnext_base_cvst`, a module that carries a ConvStem: the chain of convstem_engine.py writes the stage-0 input instead,
              and its backward takes the stage-0 gradient to the image)
  downsample  LayerNorm -> the 2x2 stride-2 conv as the GEMM's conv mode (4 taps, k_per_tap = C_in, stride 2)
  block       rart_cnx_dwconv_ln_* (7x7 depthwise conv + bias + LayerNorm, one launch) -> fc1 GEMM + exact GELU ->
              fc2 GEMM (gamma folded in) + residual, written in place over the block input
  V2 block    (ConvNeXt-V2, model.use_grn: no gamma) fc1 GEMM + GELU -> rart_cnx_grn_stats_* -> rart_cnx_grn_apply_* -> fc2 GEMM +
              residual; with the backward kept, the GELU output and the channel norms G are kept per block
  head        global average pool (rart_engine_avgpool*) -> LayerNorm -> fc GEMM (fp32 logits)
Backward: the fc dgrad GEMMs (fc2's with GELU' of the kept pre-activation in its epilogue), rart_layernorm_bwd_* against the kept
depthwise-conv output, then rart_cnx_dwconv_bwd_* (transposed 7x7 taps) adding into the residual gradient in place; the downsample's
backward is four GEMM launches, one per input parity (py, px), each scattering its output pixels with destination stride 2; the pool's
backward is rart_cnx_pool_bwd_*; the stem's is a dgrad GEMM to fp32 patches and rart_vit_unpatchify_from_f32 (patch 4, row stride 64).
A V2 block's fc2 dgrad has no epilogue; rart_cnx_grn_bwd_reduce_* then rart_cnx_grn_bwd_apply_* (GRN backward times GELU'(u), in place)
turn its output into fc1's pre-activation gradient.

precision 'bf16': bf16 storage, fp32 accumulation and statistics, every contraction on rart_conv_igemm_bf16 (the image still enters
as a hi + lo pair: the stem GEMM runs both planes as two taps).  'bf16x3' (alias 'fp32x'): the reference-precision mode, every
activation and gradient a pair of bf16 planes, every contraction the three MFMA products of rart_gemm_pair_bf16.

Torch on the forward / backward path: allocation (cached per name and shape) and the fp32 logits / gradient outputs; nothing else,
no host synchronisation."""
import ctypes

from .. import _lib
from .convstem_engine import ConvStem
from .convstem_torch import convstem_of
from .engine_base import F_GELU, F_GELU_BWD, F_GELU_KEEP, F_OUT_F32, RowEngine, act, k32, pad_k

STEM_K = 64                      # 3 x 4 x 4 = 48 columns, padded to the K granularity of both GEMMs
DS_TAPS = [(0, 0), (0, 1), (1, 0), (1, 1)]


class ConvNeXtEngine(RowEngine):
    fold_layer_scale = True          # refold: gamma folded into fc2 (the train engine keeps fc2 unscaled and applies gamma itself)

    def __init__(self, model, device='cuda', precision='bf16'):
        """precision: 'bf16' (fast path) or 'bf16x3' / 'fp32x' (reference precision: split-bf16 pairs throughout)."""
        super().__init__(device, precision)
        self.refold(model)

    def refold(self, model):
        """(Re)build every weight table from `model`'s current parameters.  fc2 carries the layer scale: W2' = gamma * W2 and
        b2' = gamma * b2 (one fp32 product per element).  The bf16 engine then rounds gamma * W2 to bf16 once, where the module
        multiplies the fp32 fc2 output by gamma; the reference-precision engine splits gamma * W2 into hi + lo, so it represents the
        fp32 product to 16 significand bits like every other weight -- no rounding beyond what the pair format already carries."""
        m, f32, tab = model, self._f32, self._table
        self.depths, self.dims = tuple(m.depths), tuple(m.dims)
        self.grn = bool(getattr(m, 'use_grn', False))          # ConvNeXt-V2: GRN after the GELU, no layer scale
        fold = self.fold_layer_scale and not self.grn
        c0 = self.dims[0]
        cvst = convstem_of(m)
        self.cvst = ConvStem(self, cvst) if cvst is not None else None                   # `convnext_base_cvst`: the stem is its chain
        if self.cvst is None:
            sw = pad_k(f32(m.stem[0].weight).reshape(c0, 48), STEM_K)                   # [c0][c*16 + r*4 + s], zero columns 48..63
            self.stem_w = self._input_table(sw, 128)                                    # bf16: [hi | hi] taps of the image pair
            self.stem_wd = tab(sw, transpose=True)                                      # [64][c0]
            self.stem_b = f32(m.stem[0].bias)
            self.stem_g, self.stem_nb = f32(m.stem[1].weight), f32(m.stem[1].bias)
        self.stages = []
        for si, st in enumerate(m.stages):
            S = dict(index=si, blocks=[])
            if si > 0:
                ln, conv = st.downsample[0], st.downsample[1]
                w = f32(conv.weight)                                                     # [cout][cin][2][2]
                cout, cin = w.shape[0], w.shape[1]
                S.update(ds_g=f32(ln.weight), ds_nb=f32(ln.bias), ds_bias=f32(conv.bias),
                         ds_w=tab(w.permute(0, 2, 3, 1).reshape(cout, 4 * cin)),         # k = (ty * 2 + tx) * cin + c
                         ds_wd=[tab(w[:, :, py, px], transpose=True) for py, px in DS_TAPS])   # per input parity: [cin][cout]
            for blk in st.blocks:
                c = blk.conv_dw.weight.shape[0]
                g = f32(blk.gamma) if fold else None
                w1 = f32(blk.mlp.fc1.weight)
                w2 = g[:, None] * f32(blk.mlp.fc2.weight) if fold else f32(blk.mlp.fc2.weight)
                S['blocks'].append(dict(
                    dw_w=f32(blk.conv_dw.weight).reshape(c, 49).t().contiguous(), dw_b=f32(blk.conv_dw.bias),
                    ng=f32(blk.norm.weight), nb=f32(blk.norm.bias),
                    fc1_w=tab(w1), fc1_b=f32(blk.mlp.fc1.bias), fc1_wd=tab(w1, transpose=True),
                    fc2_w=tab(w2), fc2_b=(g * f32(blk.mlp.fc2.bias)).contiguous() if fold else f32(blk.mlp.fc2.bias),
                    fc2_wd=tab(w2, transpose=True)))
                if self.grn:
                    S['blocks'][-1].update(grn_w=f32(blk.mlp.grn.weight), grn_b=f32(blk.mlp.grn.bias))
            self.stages.append(S)
        self.head_g, self.head_nb = f32(m.head.norm.weight), f32(m.head.norm.bias)
        self.n_classes = m.head.fc.out_features
        self.head_kpad = k32(self.n_classes)
        self.head_w = tab(m.head.fc.weight)
        self.head_wd = tab(m.head.fc.weight, self.head_kpad, transpose=True)
        self.head_b = f32(m.head.fc.bias)

    # ------------------------------------------------------------------ ConvNeXt's own precision-generic launches
    def _dwconv_ln(self, x, L, out, y, B, H, W, C):
        self._rows('cnx_dwconv_ln', act(x), L['dw_w'], L['dw_b'], L['ng'], L['nb'], act(out), act(y), B, H, W, C, 1e-6)

    def _dwconv_bwd(self, dz, L, res, dx, B, H, W, C):
        self._rows('cnx_dwconv_bwd', act(dz), L['dw_w'], act(res), act(dx), B, H, W, C)

    def _grn(self, y, L, G, z, B, P, C):
        """ConvNeXt-V2: G = the per-image channel norms of the GELU output y [B][P][C], then z = GRN(y) (z may be y)"""
        self._rows('cnx_grn_stats', act(y), G, B, P, C)
        self._rows('cnx_grn_apply', act(y), G, L['grn_w'], L['grn_b'], act(z), B, P, C, 1e-6)

    def _grn_bwd(self, g, y, u, G, L, B, P, C):
        """ConvNeXt-V2: g = the gradient of the GRN output -> in place, the gradient of fc1's pre-activation u (GRN backward times
        GELU'(u)); y and G are the forward's GELU output and channel norms"""
        torch = _lib.require_gpu()
        a = self._get('g_grn_a', (B, C), torch.float32)
        self._rows('cnx_grn_bwd_reduce', act(g), act(y), L['grn_w'], a, B, P, C)
        self._rows('cnx_grn_bwd_apply', act(g), act(y), act(u), G, a, L['grn_w'], act(g), B, P, C, 1e-6)

    def _downsample(self, x, S, out, B, H, W):
        """LayerNorm of the H x W stage output x, then the 2x2 stride-2 conv into out (H/2 x W/2)"""
        si = S['index']
        cin, cout = self.dims[si - 1], self.dims[si]
        ln = self._act('ds_ln%d' % si, (B * H * W, cin))
        self._ln(x, S['ds_g'], S['ds_nb'], ln, B * H * W, cin)
        self._conv(ln, S['ds_w'], out, B, (H // 2, W // 2), (H, W), cin, DS_TAPS, cout, (H // 2, W // 2), cout, (2, 2), (1, 1), (0, 0),
                   bias=S['ds_bias'])

    def _downsample_scatter(self, g, S, out, B, H, W):
        """backward of the 2x2 stride-2 conv: g [B][H/2][W/2][cout] -> out [B][H][W][cin], one GEMM per input parity (py, px)
        writing every second pixel of every second row (the taps do not overlap: each input pixel has exactly one)"""
        si = S['index']
        cin, cout = self.dims[si - 1], self.dims[si]
        for p, (py, px) in enumerate(DS_TAPS):
            self._conv(g, S['ds_wd'][p], out, B, (H // 2, W // 2), (H // 2, W // 2), cout, [(0, 0)], cin, (H, W), cin, (1, 1), (2, 2),
                       (py, px))

    # ------------------------------------------------------------------ forward
    def _forward(self, src, src_is_u8, mean, std, keep=False):
        torch = _lib.require_gpu()
        lib, sp = self.lib, _lib.stream_ptr()
        B, Himg, Wimg = self._image_dims(src, src_is_u8)
        if Himg % 32 or Wimg % 32:
            raise ValueError('ConvNeXt needs image sides that are multiples of 32 (got %dx%d)' % (Himg, Wimg))
        H, W = Himg // 4, Wimg // 4
        c0 = self.dims[0]
        x = self._act('x0', (B * H * W, c0))
        if self.cvst is not None:
            xs = None
            self.cvst.forward(src, src_is_u8, mean, std, B, Himg, Wimg, x)
        else:
            patches = self._get('patches', (2, B * H * W, STEM_K))
            meanf, stdf = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
            _lib.check(lib.rart_cnx_patchify(_lib.ptr(src), 1 if src_is_u8 else 0, _lib.ptr(patches[0]), _lib.ptr(patches[1]), B, Himg, Wimg,
                                             4, STEM_K, meanf, stdf, sp))
            xs = self._act('stem', (B * H * W, c0))
            self._input_gemm(patches, self.stem_w, xs, B * H * W, c0, STEM_K, bias=self.stem_b)
            self._ln(xs, self.stem_g, self.stem_nb, x, B * H * W, c0)
        saved, stage_out = [], []
        for si, S in enumerate(self.stages):
            C = self.dims[si]
            if si > 0:
                xn = self._act('x%d' % si, (B * (H // 2) * (W // 2), C))
                self._downsample(x, S, xn, B, H, W)
                stage_out.append(x)
                x, H, W = xn, H // 2, W // 2
            rows = B * H * W
            ln = self._act('ln%d' % si, (rows, C))
            hid = self._act('hid%d' % si, (rows, 4 * C))
            for bi, L in enumerate(S['blocks']):
                y = self._act('y%d_%d' % (si, bi), (rows, C)) if keep else None
                self._dwconv_ln(x, L, ln, y, B, H, W, C)
                if keep:
                    u = self._act('u%d_%d' % (si, bi), (rows, 4 * C))
                    # ConvNeXt-V2: the GELU output is the GRN backward's y, kept per block (the pair GEMM forms it from the fp32
                    # accumulator, so it cannot be recomputed bit-identically from the kept u); GRN writes the shared `hid`
                    h = self._act('h%d_%d' % (si, bi), (rows, 4 * C)) if self.grn else hid
                    if self.x3:
                        self._mm(ln, L['fc1_w'], h, rows, 4 * C, C, bias=L['fc1_b'], flags=F_GELU_KEEP, aux=u)
                    else:
                        # two launches at every batch size: the one-launch form (F_GELU_KEEP) exists only on the 256 x 256 kernel, which
                        # takes a product above a row threshold, and it applies GELU to the fp32 pre-activation where this form uses
                        # the bf16 one -- B = 256 and B = 8 would differ
                        self._mm(ln, L['fc1_w'], u, rows, 4 * C, C, bias=L['fc1_b'])
                        _lib.check(lib.rart_gelu_bf16(_lib.ptr(u), _lib.ptr(h), u.numel(), sp))
                    if self.grn:
                        G = self._get('grn_G%d_%d' % (si, bi), (B, 4 * C), torch.float32)
                        self._grn(h, L, G, hid, B, H * W, 4 * C)
                        saved.append((y, u, h, G))
                    else:
                        saved.append((y, u))
                else:
                    self._mm(ln, L['fc1_w'], hid, rows, 4 * C, C, bias=L['fc1_b'], flags=F_GELU)
                    if self.grn:
                        self._grn(hid, L, self._get('grn_G', (B, 4 * C), torch.float32), hid, B, H * W, 4 * C)
                self._mm(hid, L['fc2_w'], x, rows, C, 4 * C, bias=L['fc2_b'], res=x)       # in place: x + gamma * fc2(...)
        cl = self.dims[-1]
        pooled = self._act('pooled', (B, cl))
        self._avgpool(x, pooled, B, H * W, cl)
        pl = self._act('pooled_ln', (B, cl))
        self._ln(pooled, self.head_g, self.head_nb, pl, B, cl)
        if keep:
            self._saved = (saved, stage_out, xs, pooled, (B, Himg, Wimg))
        return self._head_logits(pl, B, cl)

    # ------------------------------------------------------------------ backward to the input
    def forward_backward(self, x01, mean, std, y, kind, y_target=None, scale=1.0):
        """-> (logits fp32, loss_indiv, d(sum_i scale*loss_i)/dx01 fp32 NCHW, pred int32); same contract as
        ResNet50Engine.forward_backward."""
        torch = _lib.require_gpu()
        cl = self.dims[-1]
        logits, loss, pred, dpl = self._forward_loss(x01, mean, std, y, kind, y_target, scale, 'g_pooled_ln', cl)
        saved, stage_out, xs, pooled, (B, Himg, Wimg) = self._saved
        dpooled = self._act('g_pooled', (B, cl))
        self._ln_bwd(dpl, pooled, self.head_g, None, dpooled, B, cl)
        H, W = Himg // 32, Wimg // 32
        n_st = len(self.stages)
        gx = self._act('g_x%d' % (n_st - 1), (B * H * W, cl))
        self._pool_bwd(dpooled, gx, B, H * W, cl)
        k = len(saved)
        for si in range(n_st - 1, -1, -1):
            S, C = self.stages[si], self.dims[si]
            rows = B * H * W
            dh = self._act('g_hid%d' % si, (rows, 4 * C))
            dln = self._act('g_ln%d' % si, (rows, C))
            dz = self._act('g_dz%d' % si, (rows, C))
            for bi in range(len(S['blocks']) - 1, -1, -1):
                L = S['blocks'][bi]
                k -= 1
                if self.grn:
                    yk, u, h, G = saved[k]
                    self._mm(gx, L['fc2_wd'], dh, rows, 4 * C, C)                              # gradient of the GRN output
                    self._grn_bwd(dh, h, u, G, L, B, H * W, 4 * C)                             # -> in place, times gelu'(u)
                else:
                    yk, u = saved[k]
                    self._mm(gx, L['fc2_wd'], dh, rows, 4 * C, C, flags=F_GELU_BWD, aux=u)   # (g W2') * gelu'(u)
                self._mm(dh, L['fc1_wd'], dln, rows, C, 4 * C)
                self._ln_bwd(dln, yk, L['ng'], None, dz, rows, C)
                self._dwconv_bwd(dz, L, gx, gx, B, H, W, C)                                   # residual + transposed 7x7, in place
            if si > 0:
                cin = self.dims[si - 1]
                gds = self._act('g_ds_ln%d' % si, (B * 4 * H * W, cin))
                self._downsample_scatter(gx, S, gds, B, 2 * H, 2 * W)
                H, W = 2 * H, 2 * W
                gprev = self._act('g_x%d' % (si - 1), (B * H * W, cin))
                self._ln_bwd(gds, stage_out[si - 1], S['ds_g'], None, gprev, B * H * W, cin)
                gx = gprev
        if self.cvst is not None:
            return logits, loss, self.cvst.backward(gx, std), pred
        c0, rows = self.dims[0], B * H * W
        gs = self._act('g_stem', (rows, c0))
        self._ln_bwd(gx, xs, self.stem_g, None, gs, rows, c0)
        dpatch = self._get('g_patch', (rows, STEM_K), torch.float32)
        self._mm(gs, self.stem_wd, dpatch, rows, STEM_K, c0, flags=F_OUT_F32)
        return logits, loss, self._unpatchify(dpatch, B, Himg, Wimg, 4, std, ld=STEM_K), pred
