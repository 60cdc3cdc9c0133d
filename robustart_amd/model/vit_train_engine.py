"""Train-mode ViT-B/16 on the HIP kernels: forward, backward to every parameter.

The training step the reference's solver runs for `vit_base` (exprs/nips_benchmark/new_adv_train/vit_base/config.yaml:
AdamW, label_smooth 0.1, drop_path_rate 0.0 -- no stochastic layers) with every FLOP on HIP kernels:

  forward / backward-to-input       ViTEngine (igemm GEMMs, fused attention forward / backward, row kernels)
  Linear weight gradients           split-K GEMM on rart_conv_igemm_bf16 over transposed operands (rart_transpose_gather_bf16,
                                    rart_wgrad_reduce_f32): EngineBase._wgrad_transposed through RowEngine._wgrad, the method behind
                                    the ResNet train engine's cross-check path as well
  Linear biases, position embedding rart_colsum_bf16
  LayerNorm gamma / beta            rart_layernorm_bwd_full_bf16 (fused with the backward to the input)

Gradients are written into the parameters' `.grad` tensors (views of the flat gradient arena, train/arena.py);
`on_grad_ready(param)` lets the arena launch a bucket's all-reduce as soon as its last gradient exists.
"""
from .. import _lib
from .engine_base import F_GELU_BWD, RowTrainMixin
from .vit_engine import ViTEngine


class ViTTrainEngine(RowTrainMixin, ViTEngine):
    # ------------------------------------------------------------------ backward to every parameter
    def backward(self, dlogits):
        """dlogits: fp32 [B][classes] = d(loss)/dlogits of the last forward().  Fills .grad of every parameter."""
        torch = _lib.require_gpu()
        lib, sp, m = self.lib, _lib.stream_ptr(), self.model
        saved, x_last, (B, Himg, Wimg, P, T) = self._saved
        D, rows = self.D, B * T
        dl = dlogits.detach().float().contiguous()
        m.head.bias.grad.copy_(dl.sum(0))
        self.on_grad_ready(m.head.bias)
        dlb = self._dlogits_rows(dl, 'g_dl', B, self.head_kpad)
        self._linear_grads(m.head, dlb, self.head_kpad, self._buf['cls'], B)
        dcls = self._get('dcls', (B, D))
        self._mm(dlb, self.head_wd, dcls, B, D, self.head_kpad)
        dx = self._get('g_x_a', (B, T, D))
        dx.zero_()
        self._ln_bwd_full(dcls, x_last, self.ng, None, dx, B, D, m.norm, strides=(D, T * D, 0, T * D))
        dqkv = self._get('g_qkv', (rows, 3 * D))
        ln = self._get('ln', (B, T, D))
        for li in range(len(self.layers) - 1, -1, -1):
            L, blk = self.layers[li], m.blocks[li]
            x_in, xm, qkv, u, att = saved[li]
            hidden = L['hidden']
            # ---- MLP: x_out = xm + fc2(gelu(fc1(LN2(xm))))
            hid = self._get('hid', (B, T, hidden))
            _lib.check(lib.rart_gelu_bf16(_lib.ptr(u), _lib.ptr(hid), u.numel(), sp))
            self._linear_grads(blk.fc2, dx, D, hid, rows)
            self._colsum(dx, D, rows, D, blk.fc2.bias.grad)
            self.on_grad_ready(blk.fc2.bias)
            dh = self._get('g_hid', (rows, hidden))
            self._mm(dx, L['fc2_wd'], dh, rows, hidden, D, flags=F_GELU_BWD, aux=u)                   # du = (dx W2) * gelu'(u)
            self._ln(xm, L['n2g'], L['n2b'], ln, rows, D)
            self._linear_grads(blk.fc1, dh, hidden, ln, rows)
            self._colsum(dh, hidden, rows, hidden, blk.fc1.bias.grad)
            self.on_grad_ready(blk.fc1.bias)
            dln = self._get('g_ln', (rows, D))
            self._mm(dh, L['fc1_wd'], dln, rows, D, hidden)
            dxm = self._get('g_xm', (B, T, D))
            self._ln_bwd_full(dln, xm, L['n2g'], dx, dxm, rows, D, blk.norm2)
            # ---- attention: xm = x_in + proj(attn(LN1(x_in)))
            self._linear_grads(blk.attn.proj, dxm, D, att, rows)
            self._colsum(dxm, D, rows, D, blk.attn.proj.bias.grad)
            self.on_grad_ready(blk.attn.proj.bias)
            datt = self._get('g_att', (rows, D))
            self._mm(dxm, L['proj_wd'], datt, rows, D, D)
            self._attention_bwd(qkv, att, datt, dqkv, B, T)
            self._ln(x_in, L['n1g'], L['n1b'], ln, rows, D)
            self._linear_grads(blk.attn.qkv, dqkv, 3 * D, ln, rows)
            self._colsum(dqkv, 3 * D, rows, 3 * D, blk.attn.qkv.bias.grad)
            self.on_grad_ready(blk.attn.qkv.bias)
            self._mm(dqkv, L['qkv_wd'], dln, rows, D, 3 * D)
            self._ln_bwd_full(dln, x_in, L['n1g'], dxm, dx, rows, D, blk.norm1)
        # ---- embeddings: x0[b][0] = cls + pos[0]; x0[b][1+p] = patch_embed(patch p) + pos[1+p]
        # derive every gradient that READS pos_embed.grad before the first on_grad_ready: with a small dist.bucket_mb the
        # {cls_token, pos_embed} bucket would otherwise start its asynchronous all-reduce (in place, on the RCCL stream)
        # while patch_embed.bias.grad is still being computed from it, and the bias would be summed across ranks twice
        pos_g = m.pos_embed.grad.view(T * D)
        self._colsum(dx, T * D, B, T * D, pos_g)
        m.cls_token.grad.view(D).copy_(pos_g[:D])
        m.patch_embed.bias.grad.copy_(m.pos_embed.grad.view(T, D)[1:].sum(0))
        self.on_grad_ready(m.pos_embed)
        self.on_grad_ready(m.cls_token)
        self.on_grad_ready(m.patch_embed.bias)
        kk = 3 * self.ps * self.ps
        patches_hi = self._buf['patches'][0]
        self._wgrad(dx.view(rows, D)[1:], D, D, patches_hi.view(B * P, kk), kk, m.patch_embed.weight.grad, B * P,
                    dz_images=(B, T, P))
        self.on_grad_ready(m.patch_embed.weight)
