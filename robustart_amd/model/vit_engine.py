"""ViT-B/16 forward and backward-to-input on the hand-written HIP kernels (evaluation of clean / corrupted images,
BASELINE config 3; the gradient step of every attack, adv/attack.py:21-22, autopgd_base.py:271-289).

One chain for both precisions on `RowEngine`'s precision-generic launches.  Every matmul -- patch embedding, qkv, proj, MLP, head --
is a GEMM launch; LayerNorm, patch extraction and the class-token / position add are small kernels; attention per (image, head) is
one fused kernel forward and one backward, or (`fused_attention` / `fused_attention_bwd` off: the cross-check) the decomposition into
batched products: S = Q K^T, soft-max rows, P V; backward S recomputed, dP = dO V^T, dQ = dS K, dK = dS^T Q, dV = P^T dO.  The dgrad
GEMMs carry GELU' in their epilogue, the LayerNorm backward adds the residual gradient.  The image enters as a hi + lo bf16 pair.
'bf16': bf16 storage, fp32 accumulation and statistics: rart_conv_igemm_bf16, rart_layernorm[_bwd]_bf16, rart_vit_attention[_bwd],
csrc/vit_aux.hip, csrc/vit_bwd.hip.  'bf16x3' (alias 'fp32x'), the reference-precision mode: every activation, gradient and weight a
hi + lo pair of bf16 planes, rart_gemm_pair_bf16 (three MFMA products per contraction), rart_layernorm[_bwd]_pair,
rart_vit_attention[_bwd]_pair, soft-max and GELU in fp32 on hi + lo (csrc/vit_pair.hip).  Above 224 tokens (`stream_attention`) the fused
attention of both precisions is the streaming one, rart_vit_attention[_bwd]_stream[_pair] (csrc/vit_stream.hip).  The LayerNorm entries of both precisions
are one kernel per direction (csrc/row_norm.hip), and so is the class-token / position add (csrc/vit_aux.hip).
A module whose patch embedding is a ConvStem (`vit_base_cvst`) runs the chain of convstem_engine.py in place of patch extraction + patch GEMM.
Reference module: robustart_amd/model/vit_torch.py."""
import os

from .. import _lib
from .convstem_engine import ConvStem
from .convstem_torch import convstem_of
from .engine_base import F_GELU_BWD, F_OUT_F32, GP_OUT_F32, RowEngine, cints, k32


class ViTEngine(RowEngine):
    def __init__(self, model, device='cuda', precision='bf16'):
        """precision: 'bf16' -- bf16 storage, fp32 accumulation (the fast path; logits within ~3e-3 of the fp32 network);
        'bf16x3' (alias 'fp32x') -- the REFERENCE-PRECISION mode: the reference evaluates and attacks ViT in fp32
        (exprs/exp/imagenet_c_loop_mini/config_vit_base.yaml:1-9 has no precision key; adv/attack.py:20-23;
        autopgd_base.py:271-289) and the north star asks for logits within 1e-4 of it."""
        super().__init__(device, precision)
        m = model
        self.D, self.H, self.ps = m.embed_dim, m.num_heads, m.patch_size
        self.hd = self.D // self.H
        self.pair_w_interleaved = os.environ.get('RART_PAIR_WIL', '0') == '1'     # see engine.py: weight tables interleaved per K step
        self.refold(model)
        self.fused_attention = True
        self.fused_attention_bwd = True      # False: the decomposition into batched products (cross-check)

    def refold(self, model):
        """(Re)build every weight table from `model`'s current parameters, in the engine's precision.  Parameters already on the
        GPU are packed there (a dozen small torch ops per layer), so the adversarial-training loop can refresh the attack engine
        every iteration, like ResNet50Engine.refold."""
        m, f32 = model, self._f32
        self._w_il = {}
        il = dict(interleave=self.pair_w_interleaved)       # `_table`: the copies of the pair tables in `_w_il`
        cvst = convstem_of(m)
        self.cvst = ConvStem(self, cvst) if cvst is not None else None                 # `vit_base_cvst`: the patch embedding is its chain
        if self.cvst is None:
            pe = m.patch_embed.weight.detach().reshape(self.D, -1)                     # [D][c*ps*ps + r*ps + s]
            self.pe_w = self._input_table(pe, 128, **il)
            self.pe_wd = self._table(pe, transpose=True, **il)
            self.pe_b = f32(m.patch_embed.bias)
        pos = f32(m.pos_embed)[0]
        self.pos = pos.contiguous()
        self.cls_pos0 = (f32(m.cls_token)[0, 0] + pos[0]).contiguous()
        self.tokens = pos.shape[0]
        self.layers = []
        for blk in m.blocks:
            L = dict(n1g=f32(blk.norm1.weight), n1b=f32(blk.norm1.bias), n2g=f32(blk.norm2.weight), n2b=f32(blk.norm2.bias),
                     hidden=blk.fc1.out_features)
            for name, lin in (('qkv', blk.attn.qkv), ('proj', blk.attn.proj), ('fc1', blk.fc1), ('fc2', blk.fc2)):
                L[name + '_w'], L[name + '_b'] = self._table(lin.weight, **il), f32(lin.bias)
                L[name + '_wd'] = self._table(lin.weight, transpose=True, **il)     # dx[rows][in] = dy[rows][out] . W
            self.layers.append(L)
        self.ng, self.nb = f32(m.norm.weight), f32(m.norm.bias)
        self.n_classes = m.head.out_features
        self.head_w = self._table(m.head.weight, **il)
        self.head_b = f32(m.head.bias)
        self.head_kpad = k32(self.n_classes)
        self.head_wd = self._table(m.head.weight, self.head_kpad, transpose=True, **il)

    # ------------------------------------------------------------------ forward
    def _forward(self, src, src_is_u8, mean, std, keep=False):
        lib, sp = self.lib, _lib.stream_ptr()
        B, Himg, Wimg = self._image_dims(src, src_is_u8)
        D, ps = self.D, self.ps
        P = (Himg // ps) * (Wimg // ps)
        T = P + 1
        assert T == self.tokens, 'image size does not match the position embedding'
        if self.x3 and not (self.fused_attention and self._pair_fused(T)):
            self._check_unfused_pair(T)
        kk = 3 * ps * ps
        rows = B * T
        x = self._act('x0' if keep else 'x', (B, T, D))
        (xh, xl), slot = self._hl(x), dict(rows_per_image=P, dst_rows_per_image=T, dst_row_off=1)      # row 0: the class token
        if self.cvst is not None:
            self.cvst.forward(src, src_is_u8, mean, std, B, Himg, Wimg, x, **slot)
        else:
            patches = self._patchify(src, src_is_u8, mean, std, B, Himg, Wimg, ps)
            self._input_gemm(patches, self.pe_w, x, B * P, D, kk, bias=self.pe_b, **slot)
        if self.x3:
            _lib.check(lib.rart_vit_add_pos_cls_pair(xh, xl, _lib.ptr(self.cls_pos0), _lib.ptr(self.pos), B, T, D, sp))
        else:
            _lib.check(lib.rart_vit_add_pos_cls(xh, _lib.ptr(self.cls_pos0), _lib.ptr(self.pos), B, T, D, sp))
        ln = self._act('ln', (B, T, D))
        saved = []
        for li, L in enumerate(self.layers):
            Hc = L['hidden']
            # keep mode stores what the backward needs: block input, post-attention stream, qkv, fc1 pre-activation
            name = 'qkv%d' % li if keep else 'qkv'
            if self.x3:
                qkv = self._get(name, (2, rows, 3 * D))
            else:
                qkv = self._get(name, (rows + 256, 3 * D), zero=True)        # bf16: slack rows, the attention reads K tiles in place
            xm = self._act('xm%d' % li, (B, T, D)) if keep else x
            att = self._act('att%d' % li if keep else 'att', (B, T, D))     # kept: delta = rowsum(dO * O) in the backward
            xo = self._act('x%d' % (li + 1), (B, T, D)) if keep else x
            self._ln(x, L['n1g'], L['n1b'], ln, rows, D)
            self._mm(ln, L['qkv_w'], qkv, rows, 3 * D, D, bias=L['qkv_b'])
            self._attention(qkv, att, B, T)
            self._mm(att, L['proj_w'], xm, rows, D, D, bias=L['proj_b'], res=x)
            self._ln(xm, L['n2g'], L['n2b'], ln, rows, D)
            hid = self._act('hid', (B, T, Hc))
            u = self._act('u%d' % li, (B, T, Hc)) if keep else None
            self._fc1_gelu(ln, L['fc1_w'], L['fc1_b'], hid, u, rows, D, Hc, keep)
            if keep:
                saved.append((x, xm, qkv, u, att))
            self._mm(hid, L['fc2_w'], xo, rows, D, Hc, bias=L['fc2_b'], res=xm)
            x = xo
        if keep:
            self._saved = (saved, x, (B, Himg, Wimg, P, T))
        cls = self._act('cls', (B, D))
        self._ln(x, self.ng, self.nb, cls, B, D, ld_in=T * D)                # the class-token row of every image
        return self._head_logits(cls, B, D)

    # ------------------------------------------------------------------ attention, per (image, head)
    RESIDENT_TOKENS = 224           # what the resident fused attention entries take: a whole (image, head) item in LDS
    stream_attention = None         # None: the streaming fused entries above RESIDENT_TOKENS; True / False forces (the cross-check)

    def _pair_fused(self, T):
        """the fused pair attention kernels take 64-wide heads; the bf16 ones have no such condition"""
        return self.hd == 64

    @staticmethod
    def _check_unfused_pair(T):
        if T > 256:
            raise ValueError('%d tokens: the unfused pair attention holds soft-max rows of at most 256 keys (rart_softmax_rows_pair); '
                             'the fused entries (64-wide heads) have no token limit' % T)

    def _streams(self, T):
        """whether the fused attention of T tokens runs on the streaming entries (K / V through LDS in chunks, any T) and not on the
        resident ones (T <= 224)"""
        return T > self.RESIDENT_TOKENS if self.stream_attention is None else bool(self.stream_attention)

    def _att_stats(self, B, T):
        """per-query statistics (max, 1 / sum, delta) between the two launches of a fused backward"""
        return self._get('att_stats', (B * self.H, k32(T), 4), _lib.require_gpu().float32)

    def _attention(self, qkv, att, B, T):
        """att[rows][D] = softmax(Q K^T / sqrt(hd)) V of one layer's qkv[rows][3D]"""
        lib, sp = self.lib, _lib.stream_ptr()
        if self.x3 and self.fused_attention and self._pair_fused(T):
            entry = lib.rart_vit_attention_stream_pair if self._streams(T) else lib.rart_vit_attention_pair
            _lib.check(entry(*self._hl(qkv), *self._hl(att), B, T, self.H, self.hd, sp))
        elif self.x3:
            self._attention_unfused_pair(qkv, att, B, T)
        elif self.fused_attention:
            entry = lib.rart_vit_attention_stream if self._streams(T) else lib.rart_vit_attention
            _lib.check(entry(_lib.ptr(qkv), _lib.ptr(att), B, T, self.H, self.hd, sp))
        else:
            self._attention_unfused(qkv, att, B, T)

    def _attention_bwd(self, qkv, att, datt, dqkv, B, T):
        """dqkv[rows][3D] from datt[rows][D] for one layer; att is the forward's output (the fused kernels' delta)"""
        lib, sp = self.lib, _lib.stream_ptr()
        if self.x3 and self.fused_attention_bwd and self._pair_fused(T):
            entry = lib.rart_vit_attention_bwd_stream_pair if self._streams(T) else lib.rart_vit_attention_bwd_pair
            _lib.check(entry(*self._hl(qkv), *self._hl(att), *self._hl(datt), *self._hl(dqkv), _lib.ptr(self._att_stats(B, T)), B, T,
                             self.H, self.hd, sp))
        elif self.x3:
            self._check_unfused_pair(T)
            self._attention_bwd_unfused_pair(qkv, datt, dqkv, B, T)
        elif self.fused_attention_bwd and self._streams(T):
            _lib.check(lib.rart_vit_attention_bwd_stream(_lib.ptr(qkv), _lib.ptr(att), _lib.ptr(datt), _lib.ptr(dqkv),
                                                         _lib.ptr(self._att_stats(B, T)), B, T, self.H, self.hd, sp))
        elif self.fused_attention_bwd:
            _lib.check(lib.rart_vit_attention_bwd(_lib.ptr(qkv), _lib.ptr(att), _lib.ptr(datt), _lib.ptr(dqkv), B, T, self.H, self.hd, sp))
        else:
            self._attention_bwd_unfused(qkv, datt, dqkv, B, T)

    # bf16 decomposition: batched rart_conv_igemm_bf16 products on bf16 score temporaries, the K / V operand a column slice of qkv
    def _scores_probs(self, qkv, B, T):
        """S = Q K^T and P = softmax(S / sqrt(d)) of one layer, batched over (image, head)"""
        D, H, hd = self.D, self.H, self.hd
        t_pad, s_ld, BH = k32(T), (T + 7) // 8 * 8, B * H              # 224: K extent of P.V; 200
        scores = self._get('scores', (BH, T, s_ld))
        probs = self._get('probs', (BH, T, t_pad))
        self._gemm(qkv, qkv[:, D:], scores, T, hd, s_ld, 3 * D, s_ld, rows_per_image=T,
                   batched=dict(n=BH, inner=H, src=(T * 3 * D, hd), wgt=(T * 3 * D, hd), dst=(H * T * s_ld, T * s_ld),
                                wgt_row_stride=3 * D))
        _lib.check(self.lib.rart_softmax_rows_bf16(_lib.ptr(scores), _lib.ptr(probs), BH * T, T, s_ld, t_pad, float(hd) ** -0.5,
                                                   _lib.stream_ptr()))
        return probs

    def _attention_unfused(self, qkv, att, B, T):
        """Q.K^T -> soft-max rows -> V transpose -> P.V; kept to cross-check the fused kernel and to exercise the batched-GEMM path
        of rart_conv_igemm_bf16."""
        D, H, hd, t_pad = self.D, self.H, self.hd, k32(T)
        probs = self._scores_probs(qkv, B, T)
        vt = self._get('vt', (B * H * hd + 128, t_pad), zero=True)
        _lib.check(self.lib.rart_vit_transpose_v(_lib.ptr(qkv), _lib.ptr(vt), B, T, H, hd, 3 * D, 2 * D, t_pad, _lib.stream_ptr()))
        self._gemm(probs, vt, att, T, t_pad, hd, t_pad, D, rows_per_image=T,
                   batched=dict(n=B * H, inner=H, src=(H * T * t_pad, T * t_pad), wgt=(H * hd * t_pad, hd * t_pad),
                                dst=(T * D, hd)))

    def _attention_bwd_unfused(self, qkv, datt, dqkv, B, T):
        """P is recomputed (S = QK^T, soft-max)."""
        lib, sp = self.lib, _lib.stream_ptr()
        D, H, hd = self.D, self.H, self.hd
        t_pad, s_ld, BH = k32(T), (T + 7) // 8 * 8, B * H
        scale = float(hd) ** -0.5
        probs = self._scores_probs(qkv, B, T)
        # dP = dO . V^T   (rows: queries, K: head_dim, columns: keys = rows of the V slice of qkv)
        dprobs = self._get('dprobs', (BH, T, s_ld))
        self._gemm(datt, qkv[:, 2 * D:], dprobs, T, hd, s_ld, D, s_ld, rows_per_image=T,
                   batched=dict(n=BH, inner=H, src=(T * D, hd), wgt=(T * 3 * D, hd), dst=(H * T * s_ld, T * s_ld),
                                wgt_row_stride=3 * D))
        ds = self._get('dscores', (BH, T, t_pad))
        _lib.check(lib.rart_softmax_bwd_rows_bf16(_lib.ptr(probs), _lib.ptr(dprobs), _lib.ptr(ds), BH * T, T, t_pad, s_ld,
                                                  t_pad, scale, sp))
        # transposed (token-contiguous) copies of K, Q, dO: [B][H][hd][t_pad]
        kt = self._get('kt', (BH * hd + 128, t_pad), zero=True)
        qt = self._get('qt', (BH * hd + 128, t_pad), zero=True)
        dot = self._get('dot', (BH * hd + 128, t_pad), zero=True)
        _lib.check(lib.rart_vit_transpose_v(_lib.ptr(qkv), _lib.ptr(kt), B, T, H, hd, 3 * D, D, t_pad, sp))
        _lib.check(lib.rart_vit_transpose_v(_lib.ptr(qkv), _lib.ptr(qt), B, T, H, hd, 3 * D, 0, t_pad, sp))
        _lib.check(lib.rart_vit_transpose_v(_lib.ptr(datt), _lib.ptr(dot), B, T, H, hd, D, 0, t_pad, sp))
        # dQ = dS . K
        self._gemm(ds, kt, dqkv, T, t_pad, hd, t_pad, 3 * D, rows_per_image=T,
                   batched=dict(n=BH, inner=H, src=(H * T * t_pad, T * t_pad), wgt=(H * hd * t_pad, hd * t_pad),
                                dst=(T * 3 * D, hd)))
        # query-contiguous copies of dS and P: [t_pad (key)][BH * t_pad (image-head, query)]
        m_all = BH * t_pad
        dst_t = self._get('ds_t', (t_pad, m_all))
        p_t = self._get('p_t', (t_pad, m_all))
        zero = cints([0])
        for src_m, dst_m in ((ds, dst_t), (probs, p_t)):
            _lib.check(lib.rart_transpose_gather_bf16(_lib.ptr(src_m), _lib.ptr(dst_m), BH, T, 1, t_pad, t_pad, 1, 1, 1, 1,
                                                      zero, zero, m_all, 0, 0, sp))
        # dK = dS^T . Q,  dV = P^T . dO   (rows: keys, K: queries)
        for a_t, w_t, col in ((dst_t, qt, D), (p_t, dot, 2 * D)):
            self._gemm(a_t, w_t, dqkv[:, col:], T, t_pad, hd, m_all, 3 * D, rows_per_image=T,
                       batched=dict(n=BH, inner=H, src=(H * t_pad, t_pad), wgt=(H * hd * t_pad, hd * t_pad),
                                    dst=(T * 3 * D, hd)))

    # pair decomposition: batched rart_gemm_pair_bf16 products with fp32 score-sized temporaries, the K / V operand at `w_off` inside
    # the qkv planes, one transpose launch per plane
    def _scores_probs_pair(self, qkv, B, T):
        """S = Q K^T (fp32) and P = softmax(S / sqrt(d)) (pair) of one layer, batched over (image, head)"""
        torch = _lib.require_gpu()
        D, H, hd = self.D, self.H, self.hd
        t_pad, s_ld, BH = k32(T), (T + 7) // 8 * 8, B * H
        scores = self._get('scores', (BH, T, s_ld), torch.float32)
        probs = self._get('probs', (2, BH, T, t_pad))
        self._gemm_pair(qkv, qkv, scores, T, s_ld, hd, 3 * D, s_ld, ldw=3 * D, flags=GP_OUT_F32, w_rows=T, w_off=D,
                        batched=dict(n=BH, inner=H, a=(T * 3 * D, hd), w=(T * 3 * D, hd), c=(H * T * s_ld, T * s_ld)))
        _lib.check(self.lib.rart_softmax_rows_pair(_lib.ptr(scores), _lib.ptr(probs[0]), _lib.ptr(probs[1]), BH * T, T, s_ld, t_pad,
                                                   float(hd) ** -0.5, _lib.stream_ptr()))
        return probs

    def _transpose_heads_pair(self, src, name, B, T, ld, off):
        """[2][B*H*hd][t_pad] token-contiguous copy of a per-head slice of a pair tensor [2][B*T][ld] (columns off + h*hd + d)"""
        H, hd, t_pad = self.H, self.hd, k32(T)
        out = self._get(name, (2, B * H * hd, t_pad))
        for p in range(2):
            _lib.check(self.lib.rart_vit_transpose_v(_lib.ptr(src[p]), _lib.ptr(out[p]), B, T, H, hd, ld, off, t_pad, _lib.stream_ptr()))
        return out

    def _attention_unfused_pair(self, qkv, att, B, T):
        D, H, hd, t_pad = self.D, self.H, self.hd, k32(T)
        probs = self._scores_probs_pair(qkv, B, T)
        vt = self._transpose_heads_pair(qkv, 'vt', B, T, 3 * D, 2 * D)
        self._gemm_pair(probs, vt, att, T, hd, t_pad, t_pad, D, ldw=t_pad, w_rows=hd,
                        batched=dict(n=B * H, inner=H, a=(H * T * t_pad, T * t_pad), w=(H * hd * t_pad, hd * t_pad), c=(T * D, hd)))

    def _attention_bwd_unfused_pair(self, qkv, datt, dqkv, B, T):
        torch = _lib.require_gpu()
        lib, sp = self.lib, _lib.stream_ptr()
        D, H, hd = self.D, self.H, self.hd
        t_pad, s_ld, BH = k32(T), (T + 7) // 8 * 8, B * H
        m_all = BH * t_pad
        probs = self._scores_probs_pair(qkv, B, T)
        dprobs = self._get('dprobs', (BH, T, s_ld), torch.float32)
        self._gemm_pair(datt, qkv, dprobs, T, s_ld, hd, D, s_ld, ldw=3 * D, flags=GP_OUT_F32, w_rows=T, w_off=2 * D,
                        batched=dict(n=BH, inner=H, a=(T * D, hd), w=(T * 3 * D, hd), c=(H * T * s_ld, T * s_ld)))       # dP = dO V^T
        ds = self._get('dscores', (2, BH, T, t_pad))
        _lib.check(lib.rart_softmax_bwd_rows_pair(_lib.ptr(probs[0]), _lib.ptr(probs[1]), _lib.ptr(dprobs), _lib.ptr(ds[0]),
                                                  _lib.ptr(ds[1]), BH * T, T, t_pad, s_ld, t_pad, float(hd) ** -0.5, sp))
        kt = self._transpose_heads_pair(qkv, 'kt', B, T, 3 * D, D)
        qt = self._transpose_heads_pair(qkv, 'qt', B, T, 3 * D, 0)
        dot = self._transpose_heads_pair(datt, 'dot', B, T, D, 0)
        hb = dict(n=BH, inner=H, a=(H * T * t_pad, T * t_pad), w=(H * hd * t_pad, hd * t_pad), c=(T * 3 * D, hd))
        self._gemm_pair(ds, kt, dqkv, T, hd, t_pad, t_pad, 3 * D, ldw=t_pad, w_rows=hd, batched=hb)                   # dQ = dS K
        # query-contiguous copies of dS and P: [t_pad (key)][BH * t_pad (image-head, query)]; queries past T are zero columns
        ds_t = self._get('ds_t', (2, t_pad, m_all))
        p_t = self._get('p_t', (2, t_pad, m_all))
        zero = cints([0])
        for src_m, dst_m in ((ds, ds_t), (probs, p_t)):
            for p in range(2):
                _lib.check(lib.rart_transpose_gather_bf16(_lib.ptr(src_m[p]), _lib.ptr(dst_m[p]), BH, T, 1, t_pad, t_pad, 1, 1, 1, 1,
                                                          zero, zero, m_all, 0, 0, sp))
        tb = dict(n=BH, inner=H, a=(H * t_pad, t_pad), w=(H * hd * t_pad, hd * t_pad), c=(T * 3 * D, hd))
        self._gemm_pair(ds_t, qt, dqkv, T, hd, t_pad, m_all, 3 * D, ldw=t_pad, w_rows=hd, batched=tb, dst_off=D)      # dK = dS^T Q
        self._gemm_pair(p_t, dot, dqkv, T, hd, t_pad, m_all, 3 * D, ldw=t_pad, w_rows=hd, batched=tb, dst_off=2 * D)  # dV = P^T dO

    # ------------------------------------------------------------------ backward to the input
    def forward_backward(self, x01, mean, std, y, kind, y_target=None, scale=1.0):
        """-> (logits fp32, loss_indiv, d(sum_i scale*loss_i)/dx01 fp32 NCHW, pred int32); same contract as
        ResNet50Engine.forward_backward."""
        torch = _lib.require_gpu()
        D = self.D
        logits, loss, pred, dcls = self._forward_loss(x01, mean, std, y, kind, y_target, scale, 'dcls', D)
        saved, x_last, (B, Himg, Wimg, P, T) = self._saved
        rows = B * T
        dx = self._act('g_x_a', (B, T, D))
        dx.zero_()                                      # only the class token receives gradient from the head
        self._ln_bwd(dcls, x_last, self.ng, None, dx, B, D, strides=(D, T * D, 0, T * D))
        dqkv = self._act('g_qkv', (rows, 3 * D))
        for li in range(len(self.layers) - 1, -1, -1):
            L = self.layers[li]
            x_in, xm, qkv, u, att = saved[li]
            Hc = L['hidden']
            dh = self._act('g_hid', (rows, Hc))
            self._mm(dx, L['fc2_wd'], dh, rows, Hc, D, flags=F_GELU_BWD, aux=u)       # du = (dx W2) * gelu'(u)
            dln = self._act('g_ln', (rows, D))
            self._mm(dh, L['fc1_wd'], dln, rows, D, Hc)
            dxm = self._act('g_xm', (B, T, D))
            self._ln_bwd(dln, xm, L['n2g'], dx, dxm, rows, D)
            datt = self._act('g_att', (rows, D))
            self._mm(dxm, L['proj_wd'], datt, rows, D, D)
            self._attention_bwd(qkv, att, datt, dqkv, B, T)
            self._mm(dqkv, L['qkv_wd'], dln, rows, D, 3 * D)
            self._ln_bwd(dln, x_in, L['n1g'], dxm, dx, rows, D)
        # patch embedding: d(patches)[b][p][c*ps*ps + r*ps + s] = dx[b][1 + p][:] . Wpe ; class token / position rows drop out.
        # bf16 patches, fp32 ones in reference precision
        if self.cvst is not None:      # the stem chain's backward, from the patch rows of dx
            return logits, loss, self.cvst.backward(dx, std, rows_per_image=P, src_rows_per_image=T, src_row_off=1), pred
        kk = 3 * self.ps * self.ps
        dpatch = self._get('g_patch', (B * P, kk), torch.float32 if self.x3 else torch.bfloat16)
        self._mm(dx, self.pe_wd, dpatch, B * P, kk, D, flags=F_OUT_F32 if self.x3 else 0, rows_per_image=P, src_rows_per_image=T,
                 src_row_off=1)
        return logits, loss, self._unpatchify(dpatch, B, Himg, Wimg, self.ps, std), pred
