"""MLP-Mixer-B/16 forward and backward-to-input on the hand-written HIP kernels (evaluation of clean / corrupted images and the
gradient step of every attack, like ViTEngine).  Reference module: robustart_amd/model/mixer_torch.py.

  stem        rart_vit_patchify -> patch GEMM (196 rows per image, no class token, no position embedding)
  block x 12  LayerNorm -> token fc1 (+ b1, GELU) -> token fc2 (+ b2, + x): the token-mixing GEMM rart_tokmix_* (csrc/mixer.hip), a
              contraction over the TOKEN axis of the [token][channel] activation with the weight table as the row operand;
              LayerNorm -> channel fc1 (+ GELU) -> fc2 (+ residual): the row GEMMs of ViT's MLP
  head        LayerNorm -> token mean (rart_engine_avgpool*) -> head GEMM (fp32 logits)
Backward: the dgrad GEMMs with GELU' of the kept pre-activations in their epilogues; the token dgrads are rart_tokmix_* with the
transposed token tables (W2^T times dx' with GELU'(u_tok), then W1^T); rart_layernorm_bwd_* adds the residual gradient; the token
mean's backward is rart_cnx_pool_bwd_*, the stem's a dgrad GEMM and rart_vit_unpatchify_*.
precision 'bf16': bf16 storage, fp32 accumulation; 'bf16x3' (alias 'fp32x'): every activation, gradient and weight a hi + lo pair of
bf16 planes, three MFMA products per contraction (rart_gemm_pair_bf16, rart_tokmix_pair), as ViTEngine's reference-precision mode.
Every dimension is read from the module."""
from .. import _lib
from .engine_base import F_GELU, F_GELU_BWD, F_GELU_KEEP, F_OUT_F32, RowEngine, k32, pad_k, pair, tokmix_desc


class MixerEngine(RowEngine):
    def __init__(self, model, device='cuda', precision='bf16'):
        super().__init__(device, precision)
        self.D, self.ps, self.T = model.embed_dim, model.patch_size, model.num_tokens
        self.refold(model)

    def refold(self, model):
        """(Re)build every weight table from `model`'s current parameters, among them the token tables W1 [Ht][T], W2 [T][Ht] and
        their transposes, K padded to a multiple of 32 with zero columns, in the engine's precision."""
        torch = _lib.require_gpu()
        m, f32 = model, self._f32

        def tok(w):                             # token table [M][K rounded up to 32], no row padding
            w = pad_k(f32(w), k32(w.shape[1])).contiguous()
            return pair(w) if self.x3 else w.to(torch.bfloat16).contiguous()
        pe = m.stem.proj.weight.detach().reshape(self.D, -1)
        self.pe_w = self._input_table(pe, 128)                                         # [hi | hi] taps of the input pair in bf16
        self.pe_wd = self._table(pe, transpose=True)
        self.pe_b = f32(m.stem.proj.bias)
        self.ng, self.nb = f32(m.norm.weight), f32(m.norm.bias)
        self.n_classes = m.head.out_features
        self.head_b = f32(m.head.bias)
        self.head_kpad = k32(self.n_classes)
        self.head_w = self._table(m.head.weight)
        self.head_wd = self._table(m.head.weight, self.head_kpad, transpose=True)
        self.layers = []
        for blk in m.blocks:
            mt, mc = blk.mlp_tokens, blk.mlp_channels
            self.layers.append(dict(
                n1g=f32(blk.norm1.weight), n1b=f32(blk.norm1.bias), n2g=f32(blk.norm2.weight), n2b=f32(blk.norm2.bias),
                tok_hidden=mt.fc1.out_features, hidden=mc.fc1.out_features,
                t1=tok(mt.fc1.weight), t1_b=f32(mt.fc1.bias), t2=tok(mt.fc2.weight), t2_b=f32(mt.fc2.bias),
                t1d=tok(mt.fc1.weight.t()), t2d=tok(mt.fc2.weight.t()),
                fc1_w=self._table(mc.fc1.weight), fc1_b=f32(mc.fc1.bias), fc1_wd=self._table(mc.fc1.weight, transpose=True),
                fc2_w=self._table(mc.fc2.weight), fc2_b=f32(mc.fc2.bias), fc2_wd=self._table(mc.fc2.weight, transpose=True)))

    # ------------------------------------------------------------------ launches
    def _tokmix(self, a, x, dst, M, K, B, bias=None, res=None, aux=None, flags=0):
        """dst_b[M][D] = a[M][K] . x_b[K][D] (+ epilogue) for the B images of dense [B][rows][D] slabs (pairs in reference precision)"""
        D = self.D
        self._launch_tokmix(tokmix_desc(a, x, dst, M, D, K, B, K * D, M * D, bias=bias, res=res, aux=aux, flags=flags,
                                        pair=self.x3), self.x3)

    # ------------------------------------------------------------------ forward
    def _forward(self, src, src_is_u8, mean, std, keep=False):
        B, Himg, Wimg = self._image_dims(src, src_is_u8)
        D, ps, T = self.D, self.ps, self.T
        assert (Himg // ps) * (Wimg // ps) == T, 'image size does not match the token-mixing MLP (%d tokens)' % T
        kk = 3 * ps * ps
        rows = B * T
        patches = self._patchify(src, src_is_u8, mean, std, B, Himg, Wimg, ps)
        x = self._act('x0' if keep else 'x', (B, T, D))
        if self.x3:
            self._input_gemm(patches, self.pe_w, x, rows, D, kk, bias=self.pe_b)
        else:                # the bf16 descriptor takes the rows image by image
            self._input_gemm(patches, self.pe_w, x, rows, D, kk, bias=self.pe_b, rows_per_image=T)
        ln = self._act('ln', (B, T, D))
        saved = []
        for li, L in enumerate(self.layers):
            Ht, Hc = L['tok_hidden'], L['hidden']
            xm = self._act('xm%d' % li, (B, T, D)) if keep else x
            xo = self._act('x%d' % (li + 1), (B, T, D)) if keep else x
            # token mixing: x' = x + W2 gelu(W1 LN1(x) + b1) + b2, per image and channel
            self._ln(x, L['n1g'], L['n1b'], ln, rows, D)
            ht = self._act('htok', (B, Ht, D))
            u_tok = self._act('utok%d' % li, (B, Ht, D)) if keep else None
            self._tokmix(L['t1'], ln, ht, Ht, T, B, bias=L['t1_b'], aux=u_tok, flags=F_GELU_KEEP if keep else F_GELU)
            self._tokmix(L['t2'], ht, xm, T, Ht, B, bias=L['t2_b'], res=x)
            # channel MLP: x'' = x' + fc2(gelu(fc1(LN2(x'))))
            self._ln(xm, L['n2g'], L['n2b'], ln, rows, D)
            hid = self._act('hid', (B, T, Hc))
            u_ch = self._act('uch%d' % li, (B, T, Hc)) if keep else None
            self._fc1_gelu(ln, L['fc1_w'], L['fc1_b'], hid, u_ch, rows, D, Hc, keep)
            self._mm(hid, L['fc2_w'], xo, rows, D, Hc, bias=L['fc2_b'], res=xm)
            if keep:
                saved.append((x, xm, u_tok, u_ch))
            x = xo
        self._ln(x, self.ng, self.nb, ln, rows, D)
        pooled = self._act('pooled', (B, D))
        self._avgpool(ln, pooled, B, T, D)
        if keep:
            self._saved = (saved, x, (B, Himg, Wimg))
        return self._head_logits(pooled, B, D)

    # ------------------------------------------------------------------ backward to the input
    def forward_backward(self, x01, mean, std, y, kind, y_target=None, scale=1.0):
        """-> (logits fp32, loss_indiv, d(sum_i scale*loss_i)/dx01 fp32 NCHW, pred int32); same contract as
        ResNet50Engine.forward_backward."""
        torch = _lib.require_gpu()
        D, T = self.D, self.T
        logits, loss, pred, dpool = self._forward_loss(x01, mean, std, y, kind, y_target, scale, 'g_pool', D)
        saved, x_last, (B, Himg, Wimg) = self._saved
        rows = B * T
        dln = self._act('g_ln', (B, T, D))
        self._pool_bwd(dpool, dln, B, T, D)
        dx = self._act('g_x', (B, T, D))
        self._ln_bwd(dln, x_last, self.ng, None, dx, rows, D)
        dxm = self._act('g_xm', (B, T, D))
        for li in range(len(self.layers) - 1, -1, -1):
            L = self.layers[li]
            x_in, xm, u_tok, u_ch = saved[li]
            Ht, Hc = L['tok_hidden'], L['hidden']
            # channel MLP: dh = (dx W2) gelu'(u_ch), dln = dh W1, dx' = LN2'(dln) + dx
            dh = self._act('g_hid', (B, T, Hc))
            self._mm(dx, L['fc2_wd'], dh, rows, Hc, D, flags=F_GELU_BWD, aux=u_ch)
            self._mm(dh, L['fc1_wd'], dln, rows, D, Hc)
            self._ln_bwd(dln, xm, L['n2g'], dx, dxm, rows, D)
            # token mixing: dht = (W2^T dx') gelu'(u_tok), dln = W1^T dht, dx = LN1'(dln) + dx'
            dht = self._act('g_htok', (B, Ht, D))
            self._tokmix(L['t2d'], dxm, dht, Ht, T, B, aux=u_tok, flags=F_GELU_BWD)
            self._tokmix(L['t1d'], dht, dln, T, Ht, B)
            self._ln_bwd(dln, x_in, L['n1g'], dxm, dx, rows, D)
        kk = 3 * self.ps * self.ps
        if self.x3:
            dpatch = self._get('g_patch32', (rows, kk), torch.float32)
            self._mm(dx, self.pe_wd, dpatch, rows, kk, D, flags=F_OUT_F32)
        else:
            dpatch = self._get('g_patch', (rows, kk))
            self._mm(dx, self.pe_wd, dpatch, rows, kk, D, rows_per_image=T)
        return logits, loss, self._unpatchify(dpatch, B, Himg, Wimg, self.ps, std), pred
