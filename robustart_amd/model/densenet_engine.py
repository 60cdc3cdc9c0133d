"""Eval-mode DenseNet-121 / -169 / -201 on the hand-written HIP kernels: forward and backward-to-input, both precisions.

The contractions are ordinary 1x1 and 3x3 convolutions on the entries ResNet50Engine uses (rart_conv_igemm_bf16 / rart_gemm_pair_bf16,
through its `_gemm`), the stem and the head are ResNet's (7x7/2 + BatchNorm + ReLU + 3x3/2 max pool; average pool + classifier), so
this engine extends ResNet50Engine and replaces the chain between them.  What DenseNet adds is in csrc/densenet.hip:

  one concat buffer per dense block, [B][h][w][C_tot]: the block's input in its first C_0 channels, layer l's 32 outputs in the channels
    [C_l, C_l + 32), C_l = C_0 + 32 l.  conv2 of a layer writes its slice in place (destination pixel stride C_tot, n_cols 32).
  dense layer l: rart_dn_preact_* (norm1's folded affine + ReLU over the prefix C_l -> a dense operand + its sign bits), the 1x1 GEMM to
    128 channels with norm2 folded in (bias + ReLU + sign bits in the epilogue), the 3x3 GEMM 128 -> 32 into the slice.
  transition: rart_dn_preact_pool2_* (affine + ReLU + 2x2 / 2 average pool, which commutes with the bias-free 1x1 after it: the GEMM
    runs on a quarter of the rows) and the 1x1 GEMM to C_tot / 2 into the next block's buffer prefix.
  tail: rart_dn_preact_* with norm5, then ResNet's average pool and head.
  backward: one gradient buffer per block, shaped like its concat buffer.  norm5's backward and every transition's backward write the
    buffer they feed (accumulate = 0); the layers run in reverse: the slice [C_l, C_l + 32) is complete once every later layer has
    added its input gradient, so it goes through conv2^T (masked by conv1's sign bits), conv1^T (norm1's scale folded into the rows of
    the transposed table) and rart_dn_preact_bwd_* with accumulate = 1 into the prefix [0, C_l).
"""
from .. import _lib
from .engine import ResNet50Engine, _Conv, _planes, _table
from .engine_base import F_MASK_BITS, F_RELU, EngineBase, check_precision, pad_rows, rows_mult


def _fold_bn(bn):
    """eval-mode BatchNorm as y = s x + t -> (s, t) fp32 on the host"""
    s = (bn.running_var.detach().float() + bn.eps).rsqrt() * bn.weight.detach().float()
    return s.contiguous(), (bn.bias.detach().float() - bn.running_mean.detach().float() * s).contiguous()


class _PreAct:
    """a pre-activation BatchNorm folded to (s, t): fp32 on the device, and on the host for the reference emulation in tests"""

    def __init__(self, bn, device):
        self.s_host, self.t_host = _fold_bn(bn)
        self.s, self.t = self.s_host.to(device), self.t_host.to(device)
        self.c = self.s_host.numel()


def _scaled_bwd_table(c, pre, device):
    """backward-to-input table of the 1x1 convolution c whose input is the pre-activation `pre`: rows [cin] of W^T scaled by pre.s, so
    the launch yields s[c] * (W^T dz)[c] and rart_dn_preact_bwd_* takes a null scale.  c.ws_folded keeps the fp32 product (tests)."""
    c.ws_folded = c.w_folded * pre.s_host.view(1, -1, 1, 1)
    return _table(lambda wb: pad_rows(wb[:, :, 0, 0].t(), rows_mult(c.cin)), _planes(c.ws_folded, c.split), device)


def check_densenet(model):
    """-> (init features, growth, mid width, block config) of a module DenseNetEngine takes; NotImplementedError otherwise"""
    f = model.features
    init, growth, mid = f.conv0.out_channels, model.growth_rate, model.bn_size * model.growth_rate
    if init != 64 or f.conv0.kernel_size != (7, 7) or f.conv0.stride != (2, 2):
        raise NotImplementedError('DenseNetEngine: the stem is ResNet\'s 7x7 / 2 convolution to 64 channels (got %d channels)' % init)
    c = init
    for i, n in enumerate(model.block_config):
        widths = [('growth rate', growth), ('bn_size * growth rate', mid), ('input width of denseblock%d' % (i + 1), c)]
        c += n * growth
        if i + 1 < len(model.block_config):
            widths.append(('output width of transition%d' % (i + 1), c // 2))
            c //= 2
        for what, v in widths:
            if v % 32 or v <= 0:
                raise NotImplementedError('DenseNetEngine: every width must be a multiple of 32, the K granularity of the GEMM entries '
                                          '(%s is %d)' % (what, v))
    return init, growth, mid, tuple(model.block_config)


class DenseNetEngine(ResNet50Engine):
    """Hand-written HIP eval engine for robustart_amd.model.densenet_torch.DenseNet, bf16 or reference precision ('fp32x')."""

    def __init__(self, model, device='cuda', precision='bf16'):
        check_precision(precision)
        assert not model.training, 'the attack / eval engine folds BatchNorm: call model.eval() first'
        self.init_features, self.growth, self.mid, self.block_config = check_densenet(model)      # before anything touches the GPU
        EngineBase.__init__(self, device, precision)
        dev, split, f = self.device, self.x3, model.features
        # the switches of ResNet50Engine that the inherited stem / head / GEMM launchers read
        self.fused_stem_fwd = self.fused_stem_bwd = self.sign_bit_masks = self.pair_gemm_kernel = True
        self.fused_stem_next_pair, self.fused_stem_next_sources, self.pair_classes = False, (), 0
        self.pair_tile, self.pair_w_interleaved = (0, 0), False
        self.blocks = []                 # no Bottlenecks
        self._build_stem(f.conv0, f.norm0)
        self.dense, self.trans = [], []
        for i, n in enumerate(self.block_config):
            layers = []
            for j in range(n):
                lay = getattr(f, 'denseblock%d' % (i + 1))['denselayer%d' % (j + 1)]
                pre = _PreAct(lay.norm1, dev)
                ca, cb = _Conv(lay.conv1, lay.norm2, dev, split), _Conv(lay.conv2, None, dev, split)
                ca.w_bwd_s = _scaled_bwd_table(ca, pre, dev)
                layers.append((pre, ca, cb))
            self.dense.append(layers)
            if i + 1 < len(self.block_config):
                tr = getattr(f, 'transition%d' % (i + 1))
                pre = _PreAct(tr.norm, dev)
                ct = _Conv(tr.conv, None, dev, split)
                ct.w_bwd_s = _scaled_bwd_table(ct, pre, dev)
                self.trans.append((pre, ct))
        self.norm5 = _PreAct(f.norm5, dev)
        self._build_head(model.classifier)
        self.small_m_fc = self.fc_in % 64 == 0      # rart_gemm_small_m_bf16 steps K by 64; other head widths go to the implicit GEMM

    def refold(self, model):
        raise NotImplementedError('refold() serves the adversarial-training loop; the DenseNet models are evaluation only: build a new '
                                  'DenseNetEngine(model, precision=%r) from the updated weights instead' % self.precision)

    # ------------------------------------------------------------------ buffers and launches
    def _op(self, name, shape):
        """a dense operand that lives for one layer: a view into the grow-only scratch buffer `name` (bf16 [shape], or the pair [2][shape])"""
        torch = _lib.require_gpu()
        n = 1
        for v in shape:
            n *= v
        lead = 2 if self.x3 else 1
        flat = self._scratch(name, lead * n * 2)[:lead * n * 2].view(torch.bfloat16)
        return flat.view((2,) + tuple(shape)) if self.x3 else flat.view(tuple(shape))

    def _slice(self, t, off):
        """the tensor t [..][C] from channel `off` of its first pixel on, flat: what a launch with a pixel stride of C reads or writes as the
        channel slice that starts at `off`"""
        return t.view(2, -1)[:, off:] if self.x3 else t.view(-1)[off:]

    def _dn(self, stem, kind, nbytes, *args):
        """one launch of rart_dn_<stem>_{bf16,pair}; args in the entry's order, an activation as a 1-tuple (t,) (hi and lo pointer in
        reference precision); profiled as `kind` with its algorithmic bytes"""
        a = []
        for v in args:
            if isinstance(v, tuple):
                t, = v
                a += [_lib.ptr(t[0]), _lib.ptr(t[1])] if self.x3 else [_lib.ptr(t)]
            else:
                a.append(_lib.ptr(v) if (v is None or hasattr(v, 'data_ptr')) else v)
        ev = self._prof_begin()
        _lib.check(getattr(self.lib, 'rart_dn_%s_%s' % (stem, 'pair' if self.x3 else 'bf16'))(*a, _lib.stream_ptr()))
        if ev is not None:
            self._prof_end(ev, 0.0, kind, nbytes)

    @property
    def _eb(self):
        """bytes per stored element"""
        return 4.0 if self.x3 else 2.0

    def _preact(self, x, ld_x, pre, y, sign, rows, c):
        self._dn('preact', 'dn_preact', rows * c * (2 * self._eb + (0.125 if sign is not None else 0)), (x,), ld_x, pre.s, pre.t, (y,), sign, rows, c)

    def _preact_bwd(self, d, bits, s, g, ld_g, accumulate, rows, c):
        self._dn('preact_bwd', 'dn_preact_bwd', rows * c * ((2 + accumulate) * self._eb + 0.125), (d,), bits, s, (g,), ld_g, accumulate, rows, c)

    def _copy(self, src, ld_src, dst, ld_dst, rows, c):
        self._dn('copy', 'dn_copy', rows * c * 2 * self._eb, (src,), ld_src, (dst,), ld_dst, rows, c)

    # ------------------------------------------------------------------ the chain
    def _geometry(self, h2, w2):
        """-> per dense block (hw, C_0, C_tot)"""
        out, c, hw = [], self.init_features, (h2, w2)
        for i, n in enumerate(self.block_config):
            out.append((hw, c, c + n * self.growth))
            c, hw = (c + n * self.growth) // 2, (hw[0] // 2, hw[1] // 2)
        return out

    def _forward(self, src, src_is_u8, mean, std, keep):
        """-> (logits fp32, acts).  keep: also write what the backward reads: the pool's argmax codes and the sign tensors -- per dense
        layer 'd%d_%d' = (sign of the pre-activated prefix, sign of conv1's output), per transition 't%d' = the full-resolution sign of
        its pre-activation, 'last_sign' = norm5's."""
        import torch
        if src_is_u8:
            B, H, W = src.shape[0], src.shape[1], src.shape[2]
        else:
            B, H, W = src.shape[0], src.shape[2], src.shape[3]
        assert H % 32 == 0 and W % 32 == 0, 'input height/width must be multiples of 32'
        x3, get, mid, gr = self.x3, self._get, self.mid, self.growth
        acts = {'in_shape': (B, H, W)}
        p1, hw, _ = self._stem_fwd(src, src_is_u8, mean, std, B, H, W, keep, keep, acts)
        geo = self._geometry(*hw)
        acts['geometry'] = geo
        cat = None
        for i, ((h, w), c0, ctot) in enumerate(geo):
            rows = B * h * w
            nxt = self._act('cat%d' % i, (B, h, w, ctot))
            if i == 0:       # the pooled stem output becomes the first 64 channels of block 1's buffer
                self._copy(p1, c0, nxt, ctot, rows, c0)
            else:            # transition i - 1: affine + ReLU + 2x2 average pool, then the 1x1 on the pooled rows into the prefix
                pre, ct = self.trans[i - 1]
                (ph, pw), _, pc = geo[i - 1]
                st = get('t%d_sign' % (i - 1), (B, ph, pw, pc // 8), torch.uint8) if keep else None
                op = self._op('dn_op', (B, h, w, pc))
                self._dn('preact_pool2', 'dn_preact_pool2', B * ph * pw * pc * (1.25 * self._eb + (0.125 if keep else 0)), (cat,), pc, pre.s,
                         pre.t, (op,), st, B, ph, pw, pc)
                self._gemm(op, ct.w_fwd, nxt, B, (h, w), (h, w), pc, pc, ct.fwd_taps, c0, (h, w), ctot, pair=x3)
                acts['t%d' % (i - 1)] = st
            cat = nxt
            ya = self._act('dn_a%d' % i, (B, h, w, mid))
            for j, (pre, ca, cb) in enumerate(self.dense[i]):
                cl = c0 + j * gr
                sx = get('d%d_%d_x_sign' % (i, j), (B, h, w, cl // 8), torch.uint8) if keep else None
                sa = get('d%d_%d_a_sign' % (i, j), (B, h, w, mid // 8), torch.uint8) if keep else None
                op = self._op('dn_op', (B, h, w, cl))
                self._preact(cat, ctot, pre, op, sx, rows, cl)
                self._gemm(op, ca.w_fwd, ya, B, (h, w), (h, w), cl, cl, ca.fwd_taps, mid, (h, w), mid, bias=ca.bias, flags=F_RELU,
                           sign_out=sa, pair=x3)
                self._gemm(ya, cb.w_fwd, self._slice(cat, cl), B, (h, w), (h, w), mid, mid, cb.fwd_taps, gr, (h, w), ctot, pair=x3)
                acts['d%d_%d' % (i, j)] = (sx, sa)
        (h, w), _, ctot = geo[-1]
        y5 = self._act('dn_y5', (B, h, w, ctot))
        s5 = get('dn_y5_sign', (B, h, w, ctot // 8), torch.uint8) if keep else None
        self._preact(cat, ctot, self.norm5, y5, s5, B * h * w, ctot)
        acts['last'], acts['last_sign'] = (y5, (h, w)), s5
        return self._head_fwd(y5, (h, w), B), acts

    def _backward(self, acts, dl, std):
        """d(loss)/d(x01) fp32 NCHW from the fp32 loss gradient dl [B][classes] and the `acts` of a keep=True forward."""
        B = acts['in_shape'][0]
        x3, mid, gr, geo = self.x3, self.mid, self.growth, acts['geometry']
        d5 = self._head_bwd(acts, dl, B)                 # classifier^T + average-pool backward, masked by norm5's ReLU
        g = None
        for i in range(len(geo) - 1, -1, -1):
            (h, w), c0, ctot = geo[i]
            rows = B * h * w
            gi = self._act('dn_g%d' % i, (B, h, w, ctot))
            if g is None:    # norm5's backward initialises the last block's buffer
                self._preact_bwd(d5, acts['last_sign'], self.norm5.s, gi, ctot, 0, rows, ctot)
            else:            # transition i: conv^T (norm's scale folded) on the pooled rows, then d / 4 under the bits initialises gi
                pre, ct = self.trans[i]
                (nh, nw), nc0, nctot = geo[i + 1]
                dt = self._op('dn_dop', (B, nh, nw, ctot))
                self._gemm(g, ct.w_bwd_s, dt, B, (nh, nw), (nh, nw), nctot, nc0, ct.bwd[0][1], ctot, (nh, nw), ctot, pair=x3)
                self._dn('preact_pool2_bwd', 'dn_preact_pool2_bwd', rows * ctot * (1.25 * self._eb + 0.125), (dt,), acts['t%d' % i], None, (gi,),
                         ctot, 0, B, h, w, ctot)
            g = gi
            dza = self._act('dn_ga%d' % i, (B, h, w, mid))
            for j in range(len(self.dense[i]) - 1, -1, -1):
                pre, ca, cb = self.dense[i][j]
                sx, sa = acts['d%d_%d' % (i, j)]
                cl = c0 + j * gr
                # the slice [cl, cl + 32) of g is complete: conv2^T under conv1's sign bits, conv1^T, then into the prefix [0, cl)
                self._gemm(self._slice(g, cl), cb.bwd[0][2], dza, B, (h, w), (h, w), ctot, gr, cb.bwd[0][1], mid, (h, w), mid, mask=sa,
                           flags=F_MASK_BITS, pair=x3)
                dop = self._op('dn_dop', (B, h, w, cl))
                self._gemm(dza, ca.w_bwd_s, dop, B, (h, w), (h, w), mid, mid, ca.bwd[0][1], cl, (h, w), cl, pair=x3)
                self._preact_bwd(dop, sx, None, g, ctot, 1, rows, cl)
        (h, w), c0, ctot = geo[0]
        dz = self._act('dn_gp1', (B, h, w, c0))
        self._copy(g, ctot, dz, c0, B * h * w, c0)
        return self._stem_bwd(acts, dz, std)
