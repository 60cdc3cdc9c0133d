"""Train-mode ConvNeXt-B and ConvNeXt-V2-B on the HIP kernels: forward, backward to every parameter.

The training step the reference's solver runs for `convnext_base` and `convnextv2_base` (exprs/nips_benchmark/{pgd,new}_adv_train/
{convnext_base,convnextv2}/config.yaml: AdamW, label_smooth 0.1, EMA, drop_path_rate 0.0 -- no stochastic layers) with every FLOP on
HIP kernels:

  forward / backward-to-input      ConvNeXtEngine's bf16 launch helpers (igemm GEMMs, fused dwconv + LayerNorm, transposed dwconv,
                                   downsample parity scatter, pool backward); fc2 runs UNFOLDED into the kept u2 and
                                   rart_cnx_layer_scale_fwd_bf16 forms x_out = x_in + gamma * u2 (the eval engine's refold puts gamma
                                   into fc2's weights instead; at gamma = 1e-6 neither gamma nor u2 could be recovered from that)
  layer scale                      rart_cnx_layer_scale_bwd_bf16: dgamma, dv = gamma * dx, fc2's bias gradient, one pass
  7x7 depthwise weight and bias    rart_cnx_dwconv_wgrad_bf16
  fc1 / fc2 / downsample weights   rart_wgrad_direct_bf16 straight from the NHWC activations (1 tap; 4 taps stride 2)
  head and stem weights            RowEngine._wgrad (split-K GEMM over transposed operands)
  Linear and conv biases           rart_colsum_bf16 (fc2's comes with the layer-scale backward)
  LayerNorm gamma / beta           rart_layernorm_bwd_full_bf16, fused with the backward to the input
  ConvNeXt-V2 block (use_grn)      no layer scale: GRN after the GELU (rart_cnx_grn_stats_bf16 into a kept G, rart_cnx_grn_apply_bf16),
                                   fc2 + bias + residual into the new x_out; kept per block: x_in, the dwconv output, u, G.  Backward:
                                   fc2's bias by rart_colsum_bf16; gelu(u) and GRN(gelu(u)) recomputed (the same kernels on the same
                                   operands: the forward's bits) for fc2's weight; fc2's dgrad with no epilogue; GRN's weight and bias
                                   and the backward's `a` by rart_cnx_grn_bwd_reduce_train_bf16; rart_cnx_grn_bwd_apply_bf16 turns
                                   fc2's dgrad in place into fc1's pre-activation gradient; the rest as above

Gradients are written into the parameters' `.grad` tensors (views of the flat gradient arena, train/arena.py); `on_grad_ready(param)`
is called once per parameter, after its gradient is final and nothing reads it again, so the arena may start that bucket's all-reduce.
Torch on the path: allocation and the head bias (a [B][classes] column sum), as in ViTTrainEngine; no host synchronisation."""
import ctypes

from .. import _lib
from .convnext_engine import DS_TAPS, STEM_K, ConvNeXtEngine
from .engine_base import F_GELU_BWD, RowTrainMixin


class ConvNeXtTrainEngine(RowTrainMixin, ConvNeXtEngine):
    fold_layer_scale = False

    def __init__(self, model, device='cuda', on_grad_ready=None):
        dp = [b.drop_path for st in model.stages for b in st.blocks if b.drop_path > 0.0]
        if dp:
            raise NotImplementedError('ConvNeXtTrainEngine: drop_path_rate > 0 (stochastic depth) is not implemented; the reference '
                                      'adversarial-training configs use 0.0 (max rate here %g)' % max(dp))
        super().__init__(model, device, on_grad_ready)
        lib = self.lib
        for si, c in enumerate(self.dims):
            ok = lib.rart_wgrad_direct_supported(c, 4 * c, 1) and lib.rart_wgrad_direct_supported(4 * c, c, 1)
            if si > 0:
                ok = ok and lib.rart_wgrad_direct_supported(self.dims[si - 1], c, 4)
            if not ok or c > 1024:
                raise ValueError('ConvNeXtTrainEngine: stage width %d is outside the weight-gradient kernels (64 or a multiple of 128, '
                                 'at most 1024)' % c)

    # ------------------------------------------------------------------ helpers
    def _ready(self, *params):
        for p in params:
            self.on_grad_ready(p)

    def _linear_wgrad(self, lin, x, dz, rows):
        """Linear weight [n_out][c_in] over NHWC rows: x [rows][c_in], dz [rows][n_out]"""
        n_out, c_in = lin.weight.shape
        self._wgrad_direct(x, dz, 1, (rows, 1), c_in, (rows, 1), n_out, n_out, [(0, 0)], 1, lin.weight.grad)
        self._ready(lin.weight)

    def _grn_block_bwd(self, gx, u, G, hid, dh, L, blk, B, P, C):
        """ConvNeXt-V2 block, fc2 and GRN: from gx (the gradient of x_out = x_in + fc2(GRN(gelu(u)))) -> fc2's and GRN's parameter
        gradients, and dh = the gradient of fc1's pre-activation u.  y = gelu(u) goes to `hid`, z = GRN(y) to `dh` until fc2's weight
        gradient has read it; then fc2's dgrad overwrites dh with the gradient of z, which the GRN backward turns in place into dh."""
        torch = _lib.require_gpu()
        lib, sp, rows, c4 = self.lib, _lib.stream_ptr(), B * P, 4 * C
        mlp = blk.mlp
        # 1. fc2 bias: the column sum of gx
        self._colsum(gx, C, rows, C, mlp.fc2.bias.grad)
        self._ready(mlp.fc2.bias)
        # 2. y = gelu(u), z = GRN(y) (the forward's bits: same kernels, same operands), fc2 weight from z and gx
        _lib.check(lib.rart_gelu_bf16(_lib.ptr(u), _lib.ptr(hid), u.numel(), sp))
        _lib.check(lib.rart_cnx_grn_apply_bf16(_lib.ptr(hid), _lib.ptr(G), _lib.ptr(L['grn_w']), _lib.ptr(L['grn_b']), _lib.ptr(dh), B, P, c4,
                                               1e-6, sp))
        self._linear_wgrad(mlp.fc2, dh, gx, rows)
        # 3. fc2 dgrad, no epilogue: g = the gradient of z
        self._mm(gx, L['fc2_wd'], dh, rows, c4, C)
        # 4. a = w * sum_p g y for the GRN backward, GRN's weight and bias gradients
        a = self._get('g_grn_a', (B, c4), torch.float32)
        need = lib.rart_cnx_grn_param_grad_workspace_bytes(B, c4)
        ws = self._scratch('grn_ws', need)
        _lib.check(lib.rart_cnx_grn_bwd_reduce_train_bf16(_lib.ptr(dh), _lib.ptr(hid), _lib.ptr(G), _lib.ptr(L['grn_w']), _lib.ptr(a),
                                                          _lib.ptr(mlp.grn.weight.grad), _lib.ptr(mlp.grn.bias.grad), B, P, c4, 1e-6, 0,
                                                          _lib.ptr(ws), need, sp))
        self._ready(mlp.grn.weight, mlp.grn.bias)
        # 5. in place: the gradient of u, GELU' included
        _lib.check(lib.rart_cnx_grn_bwd_apply_bf16(_lib.ptr(dh), _lib.ptr(hid), _lib.ptr(u), _lib.ptr(G), _lib.ptr(a), _lib.ptr(L['grn_w']),
                                                   _lib.ptr(dh), B, P, c4, 1e-6, sp))

    # ------------------------------------------------------------------ forward
    def forward(self, src, src_is_u8, mean, std):
        """train-mode forward -> fp32 logits [B][classes]; keeps what backward() needs"""
        torch = _lib.require_gpu()
        lib, sp = self.lib, _lib.stream_ptr()
        if not src_is_u8:
            src = src.detach().float().contiguous()
        B, Himg, Wimg = self._image_dims(src, src_is_u8)
        if Himg % 32 or Wimg % 32:
            raise ValueError('ConvNeXt needs image sides that are multiples of 32 (got %dx%d)' % (Himg, Wimg))
        H, W = Himg // 4, Wimg // 4
        c0 = self.dims[0]
        patches = self._get('patches', (2, B * H * W, STEM_K))
        meanf, stdf = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        _lib.check(lib.rart_cnx_patchify(_lib.ptr(src), 1 if src_is_u8 else 0, _lib.ptr(patches[0]), _lib.ptr(patches[1]), B, Himg, Wimg,
                                         4, STEM_K, meanf, stdf, sp))
        xs = self._get('t_stem', (B * H * W, c0))
        self._input_gemm(patches, self.stem_w, xs, B * H * W, c0, STEM_K, bias=self.stem_b)
        x = self._get('t_x0_0', (B * H * W, c0))
        self._ln(xs, self.stem_g, self.stem_nb, x, B * H * W, c0)
        blocks, stage_out = [], []
        for si, S in enumerate(self.stages):
            C = self.dims[si]
            if si > 0:
                xn = self._get('t_x%d_0' % si, (B * (H // 2) * (W // 2), C))
                self._downsample(x, S, xn, B, H, W)                      # keeps its LayerNorm output in 'ds_ln<si>'
                stage_out.append(x)
                x, H, W = xn, H // 2, W // 2
            rows = B * H * W
            ln = self._get('t_ln%d' % si, (rows, C))
            hid = self._get('t_hid%d' % si, (rows, 4 * C))
            for bi, L in enumerate(S['blocks']):
                y = self._get('t_y%d_%d' % (si, bi), (rows, C))
                u = self._get('t_u%d_%d' % (si, bi), (rows, 4 * C))
                xo = self._get('t_x%d_%d' % (si, bi + 1), (rows, C))    # a new buffer: the block input stays for the backward
                self._dwconv_ln(x, L, ln, y, B, H, W, C)
                self._mm(ln, L['fc1_w'], u, rows, 4 * C, C, bias=L['fc1_b'])
                _lib.check(lib.rart_gelu_bf16(_lib.ptr(u), _lib.ptr(hid), u.numel(), sp))
                if self.grn:
                    # ConvNeXt-V2: GRN in place over the GELU output, fc2 + bias + residual into the new buffer; u and G are kept,
                    # gelu(u) and GRN are recomputed bit-identically in the backward
                    G = self._get('t_grn_G%d_%d' % (si, bi), (B, 4 * C), torch.float32)
                    self._grn(hid, L, G, hid, B, H * W, 4 * C)
                    self._mm(hid, L['fc2_w'], xo, rows, C, 4 * C, bias=L['fc2_b'], res=x)
                    blocks.append((x, y, u, G))
                else:
                    gamma = self.model.stages[si].blocks[bi].gamma
                    u2 = self._get('t_u2_%d_%d' % (si, bi), (rows, C))
                    self._mm(hid, L['fc2_w'], u2, rows, C, 4 * C, bias=L['fc2_b'])             # unscaled fc2 output, kept
                    _lib.check(lib.rart_cnx_layer_scale_fwd_bf16(_lib.ptr(x), _lib.ptr(u2), _lib.ptr(gamma.detach()), _lib.ptr(xo), rows, C,
                                                                 sp))
                    blocks.append((x, y, u, u2))
                x = xo
        cl = self.dims[-1]
        pooled = self._get('t_pooled', (B, cl))
        self._avgpool(x, pooled, B, H * W, cl)
        pl = self._get('t_pooled_ln', (B, cl))
        self._ln(pooled, self.head_g, self.head_nb, pl, B, cl)
        self._saved = (blocks, stage_out, xs, pooled, pl, patches, (B, Himg, Wimg))
        return self._head_logits(pl, B, cl)

    # ------------------------------------------------------------------ backward to every parameter
    def backward(self, dlogits):
        """dlogits: fp32 [B][classes] = d(loss)/dlogits of the last forward().  Fills .grad of every parameter."""
        lib, sp, m = self.lib, _lib.stream_ptr(), self.model
        blocks, stage_out, xs, pooled, pl, patches, (B, Himg, Wimg) = self._saved
        cl, kp = self.dims[-1], self.head_kpad
        dl = dlogits.detach().float().contiguous()
        # ---- head: logits = fc(LN(mean_hw(x)))
        m.head.fc.bias.grad.copy_(dl.sum(0))
        self._ready(m.head.fc.bias)
        dlb = self._dlogits_rows(dl, 'g_dl', B, kp)
        self._wgrad(dlb, self.n_classes, kp, pl, cl, m.head.fc.weight.grad, B)
        self._ready(m.head.fc.weight)
        dpl = self._get('g_pooled_ln', (B, cl))
        self._mm(dlb, self.head_wd, dpl, B, cl, kp)
        dpooled = self._get('g_pooled', (B, cl))
        self._ln_bwd_full(dpl, pooled, self.head_g, None, dpooled, B, cl, m.head.norm)
        H, W = Himg // 32, Wimg // 32
        n_st = len(self.stages)
        gx = self._get('g_x%d' % (n_st - 1), (B * H * W, cl))
        self._pool_bwd(dpooled, gx, B, H * W, cl)
        k = len(blocks)
        for si in range(n_st - 1, -1, -1):
            S, C, stage = self.stages[si], self.dims[si], m.stages[si]
            rows = B * H * W
            dv = None if self.grn else self._get('g_dv%d' % si, (rows, C))
            hid = self._get('t_hid%d' % si, (rows, 4 * C))
            dh = self._get('g_hid%d' % si, (rows, 4 * C))
            ln = self._get('t_ln%d' % si, (rows, C))
            dln = self._get('g_ln%d' % si, (rows, C))
            dz = self._get('g_dz%d' % si, (rows, C))
            ls_need = 0 if self.grn else lib.rart_cnx_layer_scale_bwd_workspace_bytes(rows, C)
            dw_need = lib.rart_cnx_dwconv_wgrad_workspace_bytes(B, H, W, C)
            for bi in range(len(S['blocks']) - 1, -1, -1):
                L, blk = S['blocks'][bi], stage.blocks[bi]
                k -= 1
                if self.grn:
                    x_in, y, u, G = blocks[k]
                    self._grn_block_bwd(gx, u, G, hid, dh, L, blk, B, H * W, C)
                else:
                    x_in, y, u, u2 = blocks[k]
                    # 1. layer scale: x_out = x_in + gamma * u2 -> dgamma, dv = gamma * dx, fc2's bias gradient
                    ws = self._scratch('ls_ws', ls_need)
                    _lib.check(lib.rart_cnx_layer_scale_bwd_bf16(_lib.ptr(gx), _lib.ptr(u2), _lib.ptr(blk.gamma.detach()), _lib.ptr(dv),
                                                                 _lib.ptr(blk.gamma.grad), _lib.ptr(blk.mlp.fc2.bias.grad), rows, C, 0,
                                                                 _lib.ptr(ws), ls_need, sp))
                    self._ready(blk.gamma, blk.mlp.fc2.bias)
                    # 2. fc2 weight from dv and gelu(u)
                    _lib.check(lib.rart_gelu_bf16(_lib.ptr(u), _lib.ptr(hid), u.numel(), sp))
                    self._linear_wgrad(blk.mlp.fc2, hid, dv, rows)
                    # 3. fc2 dgrad with GELU' of the kept pre-activation
                    self._mm(dv, L['fc2_wd'], dh, rows, 4 * C, C, flags=F_GELU_BWD, aux=u)
                # 4. fc1 weight and bias from dh and LN(y), recomputed
                self._ln(y, L['ng'], L['nb'], ln, rows, C)
                self._linear_wgrad(blk.mlp.fc1, ln, dh, rows)
                self._colsum(dh, 4 * C, rows, 4 * C, blk.mlp.fc1.bias.grad)
                self._ready(blk.mlp.fc1.bias)
                # 5. fc1 dgrad
                self._mm(dh, L['fc1_wd'], dln, rows, C, 4 * C)
                # 6. LayerNorm against the kept conv output
                self._ln_bwd_full(dln, y, L['ng'], None, dz, rows, C, blk.norm)
                # 7. depthwise conv weight and bias
                ws = self._scratch('dw_ws', dw_need)
                _lib.check(lib.rart_cnx_dwconv_wgrad_bf16(_lib.ptr(x_in), _lib.ptr(dz), _lib.ptr(blk.conv_dw.weight.grad),
                                                          _lib.ptr(blk.conv_dw.bias.grad), B, H, W, C, 1, 0, _lib.ptr(ws), dw_need, sp))
                self._ready(blk.conv_dw.weight, blk.conv_dw.bias)
                # 8. transposed 7x7 into the residual gradient, in place: gx becomes the block input's gradient
                self._dwconv_bwd(dz, L, gx, gx, B, H, W, C)
            if si > 0:
                cin = self.dims[si - 1]
                ds_ln, conv = self._buf['ds_ln%d' % si], stage.downsample[1]
                self._colsum(gx, C, rows, C, conv.bias.grad)
                self._wgrad_direct(ds_ln, gx, B, (2 * H, 2 * W), cin, (H, W), C, C, DS_TAPS, 2, conv.weight.grad)
                self._ready(conv.bias, conv.weight)
                gds = self._get('g_ds_ln%d' % si, (B * 4 * H * W, cin))
                self._downsample_scatter(gx, S, gds, B, 2 * H, 2 * W)
                H, W = 2 * H, 2 * W
                gprev = self._get('g_x%d' % (si - 1), (B * H * W, cin))
                self._ln_bwd_full(gds, stage_out[si - 1], S['ds_g'], None, gprev, B * H * W, cin, stage.downsample[0])
                gx = gprev
        # ---- stem: x0 = LN(patches . W^T + b)
        c0, rows = self.dims[0], B * H * W
        gs = self._get('g_stem', (rows, c0))
        self._ln_bwd_full(gx, xs, self.stem_g, None, gs, rows, c0, m.stem[1])
        self._colsum(gs, c0, rows, c0, m.stem[0].bias.grad)
        self._ready(m.stem[0].bias)
        wst = self._get('g_stem_w', (c0, STEM_K), self.stem_b.dtype)
        self._wgrad(gs, c0, c0, patches[0], STEM_K, wst, rows)                 # the hi plane, K = 48 inside the 64 columns
        m.stem[0].weight.grad.view(c0, 48).copy_(wst[:, :48])
        self._ready(m.stem[0].weight)
