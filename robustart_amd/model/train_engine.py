"""Train-mode ResNet-50 on the HIP kernels: forward with batch statistics, backward to every parameter.

The training step of the reference's solver (RobustART/train/__init__.py:1 -> absent `prototype` cls_solver;
loop shape: cifar10/code/train.py:96-127; config exprs/nips_benchmark/pgd_adv_train/resnet50/config.yaml) for
`resnet50_official`: conv -> BatchNorm(batch statistics) -> ReLU bottlenecks, label-smoothed CE, gradients of all
25.6 M parameters.  PyTorch here is plumbing only (buffers, parameter storage); every FLOP and every pass over
an activation is a HIP kernel:

  contraction (forward conv, backward-to-input, weight gradient, fc)   rart_conv_igemm_bf16
  batch statistics / normalise+ReLU+residual / BatchNorm backward        rart_bn_train_forward_bf16 / _backward_bf16
  weight gradient straight from the NHWC activations                     rart_wgrad_direct_bf16
  ... for a shape that kernel does not take, or with `direct_wgrad`      EngineBase._wgrad_transposed: transposed copies of both
  off (cross-check)                                                      operands, the split-K GEMM on rart_conv_igemm_bf16
  split-K partial sums -> torch weight layout                            rart_wgrad_reduce_f32
  fp32 master weights -> bf16 igemm tables (after every optimizer step)  rart_pack_conv_weight_bf16

Gradients are written straight into the parameters' `.grad` tensors (views of the flat gradient arena,
train/arena.py); `on_grad_ready(param)` lets the arena launch a bucket's all-reduce as soon as its last gradient
exists, so the exchange overlaps the rest of the backward pass.
"""
import ctypes

from .. import _lib
from .engine_base import (F_MASK_BITS, F_MASK_RES, F_OUT_F32, EngineBase, cints, conv_desc, conv_tap_classes, lo_off, rows_mult,
                          stem_rows)


class _TConv:
    """One conv (+ its BatchNorm) in training mode: packed tables, saved activations, geometry."""

    def __init__(self, conv, bn, device, torch):
        if conv.groups != 1:
            raise NotImplementedError('ResNetTrainEngine: a grouped convolution (groups = %d) has no train-mode kernels; ResNeXt is '
                                      'evaluation only' % conv.groups)
        self.conv, self.bn = conv, bn
        self.cout, self.cin, self.r, self.s = conv.weight.shape
        self.stride, self.pad = conv.stride[0], conv.padding[0]
        self.fwd_taps, self.all_rs, classes = conv_tap_classes(self.r, self.s, self.stride, self.pad)
        bf = torch.bfloat16
        self.w_fwd = torch.zeros((self.cout + rows_mult(self.cout) - 1) // rows_mult(self.cout) * rows_mult(self.cout),
                                 self.r * self.s * self.cin, dtype=bf, device=device)
        rm = rows_mult(self.cin)
        rows_b = (self.cin + rm - 1) // rm * rm
        # (parity or None, taps [(dy,dx)], rs list, table or None)
        self.bwd = [(parity, taps, rs, torch.zeros(rows_b, len(taps) * self.cout, dtype=bf, device=device) if rs else None)
                    for parity, taps, rs in classes]
        if bn is not None:
            self.mean = torch.empty(self.cout, dtype=torch.float32, device=device)
            self.invstd = torch.empty(self.cout, dtype=torch.float32, device=device)
            self.scale_shift = torch.empty(2, self.cout, dtype=torch.float32, device=device)

    def repack(self, lib, sp):
        w = self.conv.weight
        assert w.dtype.is_floating_point and w.is_contiguous()
        wf = w.detach().float() if str(w.dtype) != 'torch.float32' else w.detach()
        rs = self.all_rs
        _lib.check(lib.rart_pack_conv_weight_bf16(wf.data_ptr(), None, self.w_fwd.data_ptr(), self.cout, self.cin, self.r, self.s,
                                                  len(rs), cints([a for a, _ in rs]), cints([b for _, b in rs]), 0,
                                                  self.w_fwd.shape[0], sp))
        for parity, taps, prs, tab in self.bwd:
            if tab is None:
                continue
            _lib.check(lib.rart_pack_conv_weight_bf16(wf.data_ptr(), None, tab.data_ptr(), self.cout, self.cin, self.r, self.s,
                                                      len(prs), cints([a for a, _ in prs]), cints([b for _, b in prs]), 1,
                                                      tab.shape[0], sp))


class ResNet50TrainEngine(EngineBase):
    def __init__(self, model, device='cuda', on_grad_ready=None, bn_momentum=None):
        super().__init__(device)
        torch = self.torch = _lib.require_gpu()
        self.model = model
        self.on_grad_ready = on_grad_ready or (lambda p: None)
        m, dev = model, self.device
        self.stem = _TConv(m.conv1, m.bn1, dev, torch)
        self.stem_w = torch.zeros(64, 2 * 7 * 32, dtype=torch.bfloat16, device=dev)
        self.blocks = []
        for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
            for blk in layer:
                ds = _TConv(blk.downsample[0], blk.downsample[1], dev, torch) if blk.downsample is not None else None
                self.blocks.append((_TConv(blk.conv1, blk.bn1, dev, torch), _TConv(blk.conv2, blk.bn2, dev, torch),
                                    _TConv(blk.conv3, blk.bn3, dev, torch), ds))
        self.n_classes, self.fc_in = m.fc.weight.shape
        self.fc_kpad = (self.n_classes + 127) // 128 * 128
        self.fc_w = torch.zeros(self.fc_kpad, self.fc_in, dtype=torch.bfloat16, device=dev)      # [1024][2048]
        self.fc_wd = torch.zeros(self.fc_in, self.fc_kpad, dtype=torch.bfloat16, device=dev)     # [2048][1024]
        self._nbt_pending = None
        self._ysign = {}
        self.direct_wgrad = True       # False: every weight gradient on `_wgrad_transposed` (rounds 1-3; cross-check)
        self.repack()

    # ------------------------------------------------------------------ tables
    def repack(self):
        """fp32 master weights -> bf16 igemm tables; call after every optimizer step."""
        torch, sp = self.torch, _lib.stream_ptr()
        convs = [c for blk in self.blocks for c in blk if c is not None]
        key = tuple(c.conv.weight.data_ptr() for c in convs)
        if all(str(c.conv.weight.dtype) == 'torch.float32' and c.conv.weight.is_contiguous() and len(c.all_rs) <= 16 for c in convs):
            # (k_pack_jobs indexes a master weight as dense [N][C][R][S]: a non-contiguous / channels_last one takes the per-conv path)
            # every table of every convolution as one job of ONE launch (rart_pack_jobs_bf16; ~110 launches of 3-10 us kernels before):
            # the job list is built once -- master weights (views into the optimizer's arena) and tables are persistent
            if getattr(self, '_pack_key', None) != key:
                jobs = []
                for c in convs:
                    for tab, rs, tr in [(c.w_fwd, c.all_rs, 0)] + [(tab, prs, 1) for _, _, prs, tab in c.bwd if tab is not None]:
                        j = _lib.PackJob()
                        j.kind, j.n_out, j.channels, j.r, j.s, j.n_taps, j.transpose, j.rows_padded = 0, c.cout, c.cin, c.r, c.s, len(rs), tr, tab.shape[0]
                        for i, (a, b) in enumerate(rs):
                            j.tap_r[i], j.tap_s[i] = a, b
                        j.weight, j.out_channel_scale, j.out = c.conv.weight.data_ptr(), None, tab.data_ptr()
                        jobs.append(j)
                arr = (_lib.PackJob * len(jobs))(*jobs)
                self._pack_jobs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
                self._pack_n, self._pack_key = len(jobs), key
            _lib.check(self.lib.rart_pack_jobs_bf16(_lib.ptr(self._pack_jobs), self._pack_n, 48, sp))
        else:
            for c in convs:
                c.repack(self.lib, sp)
        # stem forward table: a "tap" = one filter row of 8 px x 4 ch on the padded hi/lo planes (engine.py)
        wrow = stem_rows(self.model.conv1.weight.detach().float()).to(torch.bfloat16)
        self.stem_w[:, :224] = wrow
        self.stem_w[:, 224:] = wrow
        one = cints([0])
        w = self.model.fc.weight.detach()
        _lib.check(self.lib.rart_pack_conv_weight_bf16(w.data_ptr(), None, self.fc_w.data_ptr(), self.n_classes, self.fc_in, 1, 1,
                                                       1, one, one, 0, self.fc_kpad, sp))
        # backward-to-input of the classifier: rows = features, K = classes padded to fc_kpad (row stride fc_kpad)
        self.fc_wd[:, :self.n_classes] = w.t().to(torch.bfloat16)

    # ------------------------------------------------------------------ helpers
    def _get(self, name, shape, dtype=None, zero=False):
        """keyed by (name, shape, dtype), not by name: one gradient buffer name serves stages of different shapes"""
        torch = self.torch
        dtype = dtype or torch.bfloat16
        key = (name, tuple(shape), dtype)
        t = self._buf.get(key)
        if t is None:
            t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
            self._buf[key] = t
        return t

    def _conv_fwd(self, c, x, xhw, out, stats_name='bn_stats'):
        """-> (partial statistics buffer, row tiles) of the output for the BatchNorm that follows: the igemm's epilogue sums the
        columns of its 128-row tiles."""
        B = x.shape[0]
        oh, ow = xhw[0] // c.stride, xhw[1] // c.stride
        tiles = (B * oh * ow + 127) // 128
        stats = (self._scratch(stats_name, tiles * 2 * c.cout * 4), tiles)
        self._launch_conv(conv_desc(x, c.w_fwd, out, B, (oh, ow), xhw, c.cin, c.cin, c.fwd_taps, c.cout, (oh, ow), c.cout,
                                    stride=(c.stride, c.stride), stats_out=stats[0]))
        return stats

    def _conv_dgrad(self, c, dz, dz_hw, dx, dx_hw, res=None, res_mask_bits=None):
        """dx = conv^T(dz) [+ res]; res_mask_bits: the residual is masked by that 1-bit tensor in the epilogue (dx = conv^T(dz) + res . [bit]):
        the skip gradient d_out . [out > 0] without a tensor of its own."""
        B = dz.shape[0]
        for parity, taps, rs, w in c.bwd:
            if parity is None:
                self._launch_conv(conv_desc(dz, w, dx, B, dx_hw, dz_hw, c.cout, c.cout, taps, c.cin, dx_hw, c.cin, res=res, mask=res_mask_bits,
                                            flags=(F_MASK_BITS | F_MASK_RES) if res_mask_bits is not None else 0))
            else:
                ph, pw = parity
                if not taps:
                    continue
                self._launch_conv(conv_desc(dz, w, dx, B, (dx_hw[0] // 2, dx_hw[1] // 2), dz_hw, c.cout, c.cout, taps, c.cin, dx_hw,
                                            c.cin, res=res, dst_stride=(2, 2), dst_org=(ph, pw)))

    def _bn_fwd(self, c, z, y, rows, relu, res=None, stats=None):
        """stats: what `_conv_fwd` returned for z; None: the BatchNorm takes its own statistics pass over z"""
        lib, bn = self.lib, c.bn
        need = lib.rart_bn_workspace_bytes(rows, c.cout)
        ws = self._scratch('bn_ws', need)
        mom = bn.momentum if bn.momentum is not None else 0.1
        sign = None
        if relu:                         # 1 bit per element of (y > 0): what the backward reads instead of y (1/16 of its bytes)
            sign = self._get('sgn_%x' % id(c), (rows, c.cout // 8), self.torch.uint8)      # one per conv + BatchNorm (stable name: no growth when batch sizes alternate)
            self._ysign[y.data_ptr()] = sign
        _lib.check(lib.rart_bn_train_forward_bf16(
            z.data_ptr(), res.data_ptr() if res is not None else None, y.data_ptr(), _lib.ptr(sign), rows, c.cout, bn.weight.data_ptr(),
            bn.bias.data_ptr(), bn.running_mean.data_ptr() if bn.track_running_stats else None,
            bn.running_var.data_ptr() if bn.track_running_stats else None, mom, bn.eps, 1 if relu else 0,
            c.mean.data_ptr(), c.invstd.data_ptr(), c.scale_shift.data_ptr(), stats[0].data_ptr() if stats else None,
            stats[1] if stats else 0, ws.data_ptr(), need, _lib.stream_ptr()))
        if bn.track_running_stats and bn.num_batches_tracked is not None:
            if self._nbt_pending is not None:
                self._nbt_pending.append(bn.num_batches_tracked)      # one multi-tensor add at the end of forward() instead of 53 launches
            else:
                bn.num_batches_tracked += 1

    def _bn_bwd(self, c, dy, ymask, z, dz, rows, g_out=None):
        lib, bn = self.lib, c.bn
        need = lib.rart_bn_workspace_bytes(rows, c.cout)
        ws = self._scratch('bn_ws', need)
        coef = self._get('bn_coef', (3, 2048), self.torch.float32)
        bits = self._ysign.get(ymask.data_ptr()) if ymask is not None else None      # a y of this forward: its sign bits
        _lib.check(lib.rart_bn_train_backward_bf16(
            dy.data_ptr(),
            bits.data_ptr() if bits is not None else (ymask.data_ptr() if ymask is not None else None), 1 if bits is not None else 0,
            z.data_ptr(), dz.data_ptr(),
            g_out.data_ptr() if g_out is not None else None, rows, c.cout, bn.weight.data_ptr(), c.mean.data_ptr(),
            c.invstd.data_ptr(), bn.weight.grad.data_ptr(), bn.bias.grad.data_ptr(), 0, coef.data_ptr(), ws.data_ptr(),
            need, _lib.stream_ptr()))
        self.on_grad_ready(bn.weight)
        self.on_grad_ready(bn.bias)

    def _wgrad(self, dz, n_out, n_pad_cols, x, x_hw, x_c, grid_hw, taps, stride, grad, c_valid=None):
        """grad[n_out][c][taps] = sum_m dz[m][n] * x[pixel(m) + tap][c].
        dz: bf16 [B, gh, gw, n_pad_cols] (columns >= n_out are zero); x: bf16 [B, ih, iw, x_c]."""
        lib, B = self.lib, dz.shape[0]
        gh, gw = grid_hw
        if self.direct_wgrad and (c_valid is None or x_c == 4) and lib.rart_wgrad_direct_supported(x_c, n_pad_cols, len(taps)):
            # straight from the NHWC activations (csrc/wgrad_direct.hip): no transposed copies, no materialised im2col
            return self._wgrad_direct(x, dz, B, x_hw, x_c, grid_hw, n_out, n_pad_cols, taps, stride, grad, c_valid)
        self._wgrad_transposed(dz, (B, gh, gw, n_pad_cols, gh, gw), x, (B, x_hw[0], x_hw[1], x_c, gh, gw, stride, taps), n_out, grad,
                               (len(taps), c_valid if c_valid is not None else x_c, x_c))

    def _conv_wgrad(self, c, dz, dz_hw, x, x_hw):
        self._wgrad(dz, c.cout, c.cout, x, x_hw, c.cin, dz_hw, c.fwd_taps, c.stride, c.conv.weight.grad)
        self.on_grad_ready(c.conv.weight)

    # ------------------------------------------------------------------ forward
    def forward(self, src, src_is_u8, mean, std):
        torch, lib, sp = self.torch, self.lib, _lib.stream_ptr()
        if src_is_u8:
            B, H, W = src.shape[0], src.shape[1], src.shape[2]
        else:
            src = src.detach().float().contiguous()
            B, H, W = src.shape[0], src.shape[2], src.shape[3]
        assert H % 32 == 0 and W % 32 == 0
        self._nbt_pending = []
        self._ysign = {}               # activation pointer -> its sign tensor, for this forward's backward only
        hi = self._get('in_hi', (2, B, H + 8, W + 8, 4))
        _lib.check(lib.rart_engine_prep_input(_lib.ptr(src), 1 if src_is_u8 else 0, _lib.ptr(hi[0]), _lib.ptr(hi[1]), B, H, W,
                                              (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std), sp))
        h1, w1 = H // 2, W // 2
        z1 = self._get('z1', (B, h1, w1, 64))
        y1 = self._get('y1', (B, h1, w1, 64))
        tiles = (B * h1 * w1 + 127) // 128
        st = (self._scratch('bn_stats', tiles * 2 * 64 * 4), tiles)
        self._launch_conv(conv_desc(hi[0], self.stem_w, z1, B, (h1, w1), (H + 8, W + 8), 4, 32, [(r, 0) for r in range(7)] * 2, 64,
                                    (h1, w1), 64, stride=(2, 2), tap_src_off=[0] * 7 + [lo_off(hi)] * 7, stats_out=st[0]))
        self._bn_fwd(self.stem, z1, y1, B * h1 * w1, True, stats=st)
        h2, w2 = h1 // 2, w1 // 2
        p1 = self._get('p1', (B, h2, w2, 64))
        parg = self._get('p1_argmax', (B, h2, w2, 64), torch.uint8)
        _lib.check(lib.rart_engine_maxpool(_lib.ptr(y1), _lib.ptr(p1), _lib.ptr(parg), B, h1, w1, 64, sp))
        acts = {'hi': hi, 'z1': z1, 'y1': y1, 'p1': p1, 'parg': parg, 'in_shape': (B, H, W)}
        x, xhw = p1, (h2, w2)
        for bi, (ca, cb, cc, ds) in enumerate(self.blocks):
            ohw = (xhw[0] // cb.stride, xhw[1] // cb.stride)
            za = self._get('b%d_za' % bi, (B, xhw[0], xhw[1], ca.cout))
            ya = self._get('b%d_ya' % bi, (B, xhw[0], xhw[1], ca.cout))
            zb = self._get('b%d_zb' % bi, (B, ohw[0], ohw[1], cb.cout))
            yb = self._get('b%d_yb' % bi, (B, ohw[0], ohw[1], cb.cout))
            zc = self._get('b%d_zc' % bi, (B, ohw[0], ohw[1], cc.cout))
            out = self._get('b%d_out' % bi, (B, ohw[0], ohw[1], cc.cout))
            st = self._conv_fwd(ca, x, xhw, za)
            self._bn_fwd(ca, za, ya, B * xhw[0] * xhw[1], True, stats=st)
            st = self._conv_fwd(cb, ya, xhw, zb)
            rows_o = B * ohw[0] * ohw[1]
            self._bn_fwd(cb, zb, yb, rows_o, True, stats=st)
            st_c = self._conv_fwd(cc, yb, ohw, zc)
            zd = None
            if ds is not None:
                zd = self._get('b%d_zd' % bi, (B, ohw[0], ohw[1], cc.cout))
                sk = self._get('b%d_sk' % bi, (B, ohw[0], ohw[1], cc.cout))
                st = self._conv_fwd(ds, x, xhw, zd, stats_name='bn_stats_ds')
                self._bn_fwd(ds, zd, sk, rows_o, False, stats=st)
            else:
                sk = x
            self._bn_fwd(cc, zc, out, rows_o, True, res=sk, stats=st_c)
            acts['b%d' % bi] = (x, xhw, za, ya, zb, yb, zc, zd, out, ohw)
            x, xhw = out, ohw
        pooled = self._get('pooled', (B, self.fc_in))
        _lib.check(lib.rart_engine_avgpool(_lib.ptr(x), _lib.ptr(pooled), B, xhw[0] * xhw[1], self.fc_in, sp))
        logits = torch.empty(B, self.n_classes, dtype=torch.float32, device=self.device)
        self._launch_conv(conv_desc(pooled, self.fc_w, logits, B, (1, 1), (1, 1), self.fc_in, self.fc_in, [(0, 0)], self.n_classes,
                                    (1, 1), self.n_classes, bias=self.model.fc.bias.detach(), flags=F_OUT_F32))
        acts['last'], acts['pooled'] = (x, xhw), pooled
        self.acts = acts
        pending, self._nbt_pending = self._nbt_pending, None
        if pending:
            torch._foreach_add_(pending, 1)
        return logits

    # ------------------------------------------------------------------ backward to every parameter
    def backward(self, dlogits):
        """dlogits: fp32 [B][classes] = d(loss)/dlogits.  Fills .grad of every parameter (overwrites)."""
        torch, lib, sp, acts = self.torch, self.lib, _lib.stream_ptr(), self.acts
        B, H, W = acts['in_shape']
        fc = self.model.fc
        dl = dlogits.detach().float().contiguous()
        fc.bias.grad.copy_(dl.sum(0))
        self.on_grad_ready(fc.bias)
        dlb = self._dlogits_rows(dl, 'dl_bf16', B, self.fc_kpad)
        pooled = acts['pooled']
        # classifier weight gradient: [classes][features] = dl^T . pooled  (1x1 "conv" over B pixels)
        self._wgrad(dlb.view(B, 1, 1, self.fc_kpad), self.n_classes, self.fc_kpad, pooled.view(B, 1, 1, self.fc_in), (1, 1),
                    self.fc_in, (1, 1), [(0, 0)], 1, fc.weight.grad)
        self.on_grad_ready(fc.weight)
        dpool = self._get('dpool', (B, self.fc_in))
        self._launch_conv(conv_desc(dlb, self.fc_wd, dpool, B, (1, 1), (1, 1), self.fc_kpad, self.fc_kpad, [(0, 0)], self.fc_in,
                                    (1, 1), self.fc_in))
        xl, xlhw = acts['last']
        d_out = self._get('g_out_a', tuple(xl.shape))
        _lib.check(lib.rart_engine_avgpool_bwd(_lib.ptr(xl), _lib.ptr(dpool), _lib.ptr(d_out), B, xlhw[0] * xlhw[1],
                                               self.fc_in, sp))
        for bi in range(len(self.blocks) - 1, -1, -1):
            ca, cb, cc, ds = self.blocks[bi]
            x, xhw, za, ya, zb, yb, zc, zd, out, ohw = acts['b%d' % bi]
            rows_o, rows_i = B * ohw[0] * ohw[1], B * xhw[0] * xhw[1]
            dzc = self._get('g_zc', tuple(zc.shape))
            g = self._get('g_skip', tuple(zc.shape)) if ds is not None else None      # the skip gradient a projection reads
            self._bn_bwd(cc, d_out, out, zc, dzc, rows_o, g_out=g)
            self._conv_wgrad(cc, dzc, ohw, yb, ohw)
            dyb = self._get('g_yb', tuple(yb.shape))
            self._conv_dgrad(cc, dzc, ohw, dyb, ohw)
            dzb = self._get('g_zb', tuple(zb.shape))
            self._bn_bwd(cb, dyb, yb, zb, dzb, rows_o)
            self._conv_wgrad(cb, dzb, ohw, ya, xhw)
            dya = self._get('g_ya', tuple(ya.shape))
            if cb.stride == 2:
                dya.zero_()                      # parity classes without taps receive no gradient
            self._conv_dgrad(cb, dzb, ohw, dya, xhw)
            dza = self._get('g_za', tuple(za.shape))
            self._bn_bwd(ca, dya, ya, za, dza, rows_i)
            self._conv_wgrad(ca, dza, xhw, x, xhw)
            dx = self._get('g_x_%d' % (bi % 2), tuple(x.shape))
            if ds is None:
                # the identity skip's gradient d_out . [out > 0] is formed in the dgrad epilogue from d_out and the sign bits of `out`
                self._conv_dgrad(ca, dza, xhw, dx, xhw, res=d_out, res_mask_bits=self._ysign[out.data_ptr()])
            else:
                self._conv_dgrad(ca, dza, xhw, dx, xhw)
                dzd = self._get('g_zd', tuple(zd.shape))
                self._bn_bwd(ds, g, None, zd, dzd, rows_o)
                self._conv_wgrad(ds, dzd, ohw, x, xhw)
                # accumulate the projection skip (a 1x1 stride-2 conv reaches only the even/even pixels)
                self._conv_dgrad(ds, dzd, ohw, dx, xhw, res=dx)
            d_out = dx
        # stem: max-pool backward (applies y1's ReLU mask), BatchNorm backward, weight gradient on the padded hi plane
        y1, z1 = acts['y1'], acts['z1']
        h1, w1 = H // 2, W // 2
        dy1 = self._get('g_y1', tuple(y1.shape))
        _lib.check(lib.rart_engine_maxpool_bwd(_lib.ptr(y1), _lib.ptr(acts['parg']), _lib.ptr(d_out), _lib.ptr(dy1), B, h1, w1,
                                               64, sp))
        dz1 = self._get('g_z1', tuple(z1.shape))
        self._bn_bwd(self.stem, dy1, y1, z1, dz1, B * h1 * w1)
        taps = [(r, s) for r in range(7) for s in range(7)]    # hi plane holds the image at offset (3, 3)
        self._wgrad(dz1, 64, 64, acts['hi'][0], (H + 8, W + 8), 4, (h1, w1), taps, 2, self.model.conv1.weight.grad, c_valid=3)
        self.on_grad_ready(self.model.conv1.weight)
