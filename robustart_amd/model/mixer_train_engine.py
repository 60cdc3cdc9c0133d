"""Train-mode MLP-Mixer-B/16 on the HIP kernels: forward, backward to every parameter.

The training step the reference's solver runs for `mixer_b16_224` (exprs/nips_benchmark/pgd_adv_train/mixer_B16_224/config.yaml:
AdamW, label_smooth 0.1, drop rates 0 -- no stochastic layers) with every FLOP on HIP kernels:

  forward / backward-to-input       MixerEngine (token-mixing GEMMs rart_tokmix_bf16, row GEMMs, row kernels)
  token-mixing weight gradients     rart_tokmix_wgrad_bf16 (csrc/mixer_train.hip): both operands read as they lie, channel contiguous,
                                    split over images, folded by rart_wgrad_reduce_f32 -- no transposed copy of an activation
  token-mixing bias gradients       rart_tok_rowsum_bf16
  channel MLP, head, stem weights   the split-K GEMM over transposed operands (RowEngine._wgrad), the ViT train engine's path
  their biases                      rart_colsum_bf16
  LayerNorm gamma / beta            rart_layernorm_bwd_full_bf16 (fused with the backward to the input)

gelu(u_tok), gelu(u_ch), LN1(x) and LN2(x') are recomputed from the kept pre-activations and block inputs (rart_gelu_bf16,
rart_layernorm_bf16) into the forward's buffers.  Gradients are written into the parameters' `.grad` tensors (views of the flat
gradient arena, train/arena.py); `on_grad_ready(param)` lets the arena launch a bucket's all-reduce as soon as its last gradient exists.
"""
import ctypes

from .. import _lib
from .engine_base import F_GELU_BWD, RowTrainMixin, tokmix_wgrad_desc, wgrad_split_tokens
from .mixer_engine import MixerEngine


class MixerTrainEngine(RowTrainMixin, MixerEngine):
    # ------------------------------------------------------------------ token-mixing parameter gradients
    def _tok_wgrad(self, p, q, M, N, B, grad, accumulate=0):
        """grad[M][N] (+)= sum_b sum_d p_b[m][d] q_b[n][d] for dense bf16 slabs p [B][M][D], q [B][N][D]: rart_tokmix_wgrad_bf16 over
        `wgrad_split_tokens` splits of the batch, then rart_wgrad_reduce_f32"""
        lib, sp, D = self.lib, _lib.stream_ptr(), self.D
        splits, per = wgrad_split_tokens(B, M, N, self.wgrad_target_wgs)
        ld = (M + 7) // 8 * 8
        part = self._scratch('tokwg_part', splits * N * ld * 4)
        ev = self._prof_begin()
        _lib.check(lib.rart_tokmix_wgrad_bf16(ctypes.byref(tokmix_wgrad_desc(p, q, part, M, N, D, B, splits, per, ld)), sp))
        if ev is not None:
            self._prof_end(ev, 2.0 * B * M * N * D, 'tok_wgrad')
        ev = self._prof_begin()
        _lib.check(lib.rart_wgrad_reduce_f32(_lib.ptr(part), splits, 1, N, N, M, ld, _lib.ptr(grad), accumulate, sp))
        if ev is not None:
            self._prof_end(ev, 0.0, 'tok_wgrad_reduce')

    def _tok_rowsum(self, x, M, B, out, accumulate=0):
        """out[M] (+)= sum_b sum_d x_b[m][d] for dense bf16 slabs x [B][M][D]"""
        lib, D = self.lib, self.D
        need = lib.rart_tok_rowsum_workspace_bytes(M, B)
        ws = self._scratch('tokrs_ws', need)
        ev = self._prof_begin()
        _lib.check(lib.rart_tok_rowsum_bf16(_lib.ptr(x), M, D, B, M * D, _lib.ptr(out), accumulate, _lib.ptr(ws), need, _lib.stream_ptr()))
        if ev is not None:
            self._prof_end(ev, 0.0, 'tok_rowsum')

    # ------------------------------------------------------------------ backward to every parameter
    def backward(self, dlogits):
        """dlogits: fp32 [B][classes] = d(loss)/dlogits of the last forward().  Fills .grad of every parameter."""
        lib, sp, m = self.lib, _lib.stream_ptr(), self.model
        saved, x_last, (B, Himg, Wimg) = self._saved
        D, T, kp = self.D, self.T, self.head_kpad
        rows = B * T
        dl = dlogits.detach().float().contiguous()
        m.head.bias.grad.copy_(dl.sum(0))
        self.on_grad_ready(m.head.bias)
        dlb = self._dlogits_rows(dl, 'g_dl', B, kp)
        self._linear_grads(m.head, dlb, kp, self._buf['pooled'], B)
        dpool = self._get('g_pool', (B, D))
        self._mm(dlb, self.head_wd, dpool, B, D, kp)
        dln = self._get('g_ln', (B, T, D))
        self._pool_bwd(dpool, dln, B, T, D)
        dx = self._get('g_x', (B, T, D))
        self._ln_bwd_full(dln, x_last, self.ng, None, dx, rows, D, m.norm)
        dxm = self._get('g_xm', (B, T, D))
        ln = self._get('ln', (B, T, D))
        for li in range(len(self.layers) - 1, -1, -1):
            L, blk = self.layers[li], m.blocks[li]
            x_in, xm, u_tok, u_ch = saved[li]
            Ht, Hc = L['tok_hidden'], L['hidden']
            mt, mc = blk.mlp_tokens, blk.mlp_channels
            # ---- channel MLP: x_out = xm + fc2(gelu(fc1(LN2(xm))))
            hid = self._get('hid', (B, T, Hc))
            _lib.check(lib.rart_gelu_bf16(_lib.ptr(u_ch), _lib.ptr(hid), u_ch.numel(), sp))
            self._linear_grads(mc.fc2, dx, D, hid, rows)
            self._colsum(dx, D, rows, D, mc.fc2.bias.grad)
            self.on_grad_ready(mc.fc2.bias)
            dh = self._get('g_hid', (B, T, Hc))
            self._mm(dx, L['fc2_wd'], dh, rows, Hc, D, flags=F_GELU_BWD, aux=u_ch)                  # du = (dx W2) * gelu'(u)
            self._ln(xm, L['n2g'], L['n2b'], ln, rows, D)
            self._linear_grads(mc.fc1, dh, Hc, ln, rows)
            self._colsum(dh, Hc, rows, Hc, mc.fc1.bias.grad)
            self.on_grad_ready(mc.fc1.bias)
            self._mm(dh, L['fc1_wd'], dln, rows, D, Hc)
            self._ln_bwd_full(dln, xm, L['n2g'], dx, dxm, rows, D, blk.norm2)
            # ---- token mixing: xm = x_in + W2 gelu(W1 LN1(x_in) + b1) + b2, per image and channel
            htok = self._get('htok', (B, Ht, D))
            _lib.check(lib.rart_gelu_bf16(_lib.ptr(u_tok), _lib.ptr(htok), u_tok.numel(), sp))
            self._tok_wgrad(dxm, htok, T, Ht, B, mt.fc2.weight.grad)                              # dW2[t][h] = sum dx'[t][d] gelu(u)[h][d]
            self.on_grad_ready(mt.fc2.weight)
            self._tok_rowsum(dxm, T, B, mt.fc2.bias.grad)
            self.on_grad_ready(mt.fc2.bias)
            dht = self._get('g_htok', (B, Ht, D))
            self._tokmix(L['t2d'], dxm, dht, Ht, T, B, aux=u_tok, flags=F_GELU_BWD)                 # du = (W2^T dx') * gelu'(u)
            self._ln(x_in, L['n1g'], L['n1b'], ln, rows, D)
            self._tok_wgrad(dht, ln, Ht, T, B, mt.fc1.weight.grad)                                # dW1[h][t] = sum du[h][d] LN1(x)[t][d]
            self.on_grad_ready(mt.fc1.weight)
            self._tok_rowsum(dht, Ht, B, mt.fc1.bias.grad)
            self.on_grad_ready(mt.fc1.bias)
            self._tokmix(L['t1d'], dht, dln, T, Ht, B)
            self._ln_bwd_full(dln, x_in, L['n1g'], dxm, dx, rows, D, blk.norm1)
        # ---- stem: x0 = patch_embed(patches) + bias
        self._colsum(dx, D, rows, D, m.stem.proj.bias.grad)
        self.on_grad_ready(m.stem.proj.bias)
        kk = 3 * self.ps * self.ps
        self._linear_grads(m.stem.proj, dx.view(rows, D), D, self._buf['patches'][0].view(rows, kk), rows)
