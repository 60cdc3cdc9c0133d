"""Eval-mode ResNet-50 on the hand-written HIP kernels: forward and backward-to-input.

This is the `f_model(x)` + autograd step that every iteration of the reference's attacks
performs (RobustART/noise/utils/adv/attack.py:21-22; Attacks/autoattack/autopgd_base.py:271-289,
367-384; Attacks/imfgsm_attack.py:82-84) and the clean / corrupted evaluation forward
(SURVEY.md 3.5).  Model definition: RobustART/model/__init__.py:1 -> absent submodule; the public
ResNet-50 v1.5 (robustart_amd/model/resnet_torch.py is the plain-PyTorch statement of it).

Host side (this file, PyTorch as plumbing only): fold BatchNorm (eval mode) into conv weight/bias,
lay the weights out for the implicit-GEMM kernel (forward: [Cout][tap][Cin]; backward-to-input:
[Cin][tap][Cout], one table per input-parity class for stride-2 convs), own the activation / gradient
buffers, and sequence the C-ABI calls.  Device side: rart_conv_igemm_bf16 (every conv, fc, and their
backward), rart_engine_* (stem input prep, pools, col2im), rart_logit_loss.  Two precisions, one chain (`ResNet50Engine`):
bf16 storage with fp32 accumulation, where the fp32 pixels enter the stem as a hi+lo bf16 pair so eps-sized perturbations are
kept; or reference precision, where every tensor is such a pair and rart_gemm_pair_bf16 / the rart_*_pair entries take the
place of their bf16 namesakes.
"""
import ctypes
import os as _os

from .. import _lib
from .engine_base import (F_MASK_BITS, F_OUT_F32, F_PAIR, F_RELU, EngineBase, cints as _cints, conv_desc, conv_tap_classes,
                          gemm_pair_cls_desc, gemm_pair_desc, interleave_k32, lo_off, pad_k, pad_rows, rows_mult, pair, split_hi_lo, stem_rows)


def _bf16(t):
    import torch
    return t.to(torch.bfloat16).contiguous()


def _planes(w, split):
    """the bf16-exact fp32 pieces a weight table is built from: (hi,) with hi = bf16(w), the values the bf16 kernels see; in reference
    precision (hi, lo) with w = hi + lo (two bf16 pieces, 16 significand bits)"""
    hi, lo = split_hi_lo(w)
    return (hi.float(), lo.float()) if split else (hi.float(),)


def _table(build, planes, device):
    """the bf16 table build(hi) [rows][K], or in reference precision its rows as [hi | lo | hi]: the concatenation that matches the three
    products x_hi.w_hi + x_hi.w_lo + x_lo.w_hi (F_PAIR)"""
    import torch
    t = [build(p) for p in planes]
    return _bf16(torch.cat(t + t[:1], 1) if len(t) == 2 else t[0]).to(device)


def _cat_k(t1, k1, t2, k2):
    """two [rows][hi | lo | hi] tables of `_Conv(split=True)`, K = k1 and k2, as ONE such table whose rows are [T1 | T2] along K: the
    table of a two-source rart_gemm_pair_bf16 launch (hi = [T1_hi | T2_hi], lo = [T1_lo | T2_lo], row stride 3 (k1 + k2))"""
    import torch
    assert t1.shape == (t2.shape[0], 3 * k1) and t2.shape[1] == 3 * k2
    return torch.cat([t[:, i * k:(i + 1) * k] for i in range(3) for t, k in ((t1, k1), (t2, k2))], 1).contiguous()


def fold_shortcut_tables(ca, cc, ds):
    """Reference precision, a Bottleneck (conv1 ca, conv3 cc) with the 1x1 projection shortcut ds: the tables that fold the shortcut into
    the launch it is added in.  ds.w_cat = rows [W3 | Wds] and ds.bias_cat = b3 + bds: yc = relu(W3 . yb + Wds . x_strided + bias_cat) is
    one accumulation of a two-source launch.  A stride-1 shortcut also gets ds.w_cat_bwd = rows [W1^T | Wds^T]: dx = mask(W1^T . dza +
    Wds^T . dz).  -> whether the block has the form (1x1 convolutions, power-of-two K of the first source)."""
    pow2 = lambda k: k >= 32 and (k & (k - 1)) == 0                      # noqa: E731
    if not (cc.r == 1 and cc.stride == 1 and ds.r == 1 and ds.cout == cc.cout and pow2(cc.cin) and ds.cin % 32 == 0):
        return False
    ds.w_cat = _cat_k(cc.w_fwd, cc.cin, ds.w_fwd, ds.cin)
    ds.bias_cat = (cc.bias + ds.bias).contiguous()
    if ds.stride == 1 and ca.r == 1 and ca.stride == 1 and ca.cin == ds.cin and pow2(ca.cout) and ds.cout % 32 == 0:
        ds.w_cat_bwd = _cat_k(ca.bwd[0][2], ca.cout, ds.bwd[0][2], ds.cout)
    return True


def _cat_classes(tabs):
    """[rows][hi | lo | hi] tables of `_Conv(split=True)` with K = k_0, k_1, ... -> (ONE such table whose rows hold the slices side by side
    along K, class by class: hi = [T0_hi | T1_hi | ...], lo likewise, row stride 3 sum(k); the first column of every slice): the table of a
    rart_gemm_pair_classes_bf16 launch"""
    import torch
    ks = [t.shape[1] // 3 for t in tabs]
    assert all(t.shape == (tabs[0].shape[0], 3 * k) for t, k in zip(tabs, ks))
    tab = torch.cat([t[:, i * k:(i + 1) * k] for i in range(3) for t, k in zip(tabs, ks)], 1).contiguous()
    return tab, [sum(ks[:i]) for i in range(len(ks))]


def class_tables(ca, cb, ds):
    """Reference precision, the class-ordered tables of a stride-2 first block (conv1 ca, 3x3 cb, projection shortcut ds), for launches
    that run the four input-parity classes of a stride-2 backward in one grid.  cb.cls_bwd = (table, [(taps, k_off, parity)]): the four
    per-class tables of cb.bwd as one.  ds.cls_bwd = the same for dx = mask(W1^T . dza + Wds^T . dz): conv1^T read at the four parities of
    dza, the class (0, 0) with the shortcut^T as its second source (rows [W1^T | Wds^T]); the other three slices are W1^T again."""
    pow2 = lambda k: k >= 32 and (k & (k - 1)) == 0                      # noqa: E731
    if cb.groups == 1 and cb.stride == 2 and all(taps and tab is not None for _, taps, tab in cb.bwd) and sum(len(t) for _, t, _ in cb.bwd) <= 16 and pow2(cb.cout):
        tab, offs = _cat_classes([t for _, _, t in cb.bwd])
        cb.cls_bwd = (tab, [(taps, off, parity) for (parity, taps, _), off in zip(cb.bwd, offs)])
    if ds is not None and ds.stride == 2 and ds.r == 1 and ca.r == 1 and ca.stride == 1 and ca.cin == ds.cin and pow2(ca.cout) and ds.cout % 32 == 0:
        w1, wd = ca.bwd[0][2], ds.bwd[0][2]
        tab, offs = _cat_classes([_cat_k(w1, ca.cout, wd, ds.cout), w1, w1, w1])
        ds.cls_bwd = (tab, [([(ph, pw)], off, (ph, pw)) for (ph, pw), off in zip(((0, 0), (0, 1), (1, 0), (1, 1)), offs)])


class _Conv:
    """One folded conv layer: forward table + backward-to-input tables, in bf16 or (split) as [hi | lo | hi] rows."""

    def __init__(self, conv, bn, device, split=False):
        import torch
        w = conv.weight.detach().float()
        if bn is not None:
            inv = (bn.running_var.detach().float() + bn.eps).rsqrt() * bn.weight.detach().float()
            w = w * inv.view(-1, 1, 1, 1)
            b = bn.bias.detach().float() - bn.running_mean.detach().float() * inv
        else:
            b = conv.bias.detach().float() if conv.bias is not None else torch.zeros(w.shape[0])
        self.cout, self.cin, self.r, self.s = w.shape
        self.groups = conv.groups
        self.cin *= self.groups              # (a grouped weight is [cout][cin / groups][r][s])
        self.stride = conv.stride[0]
        self.pad = pad = conv.padding[0]
        self.w_folded = w                    # fp32, for the reference emulation in tests
        self.b_folded = b
        self.bias = b.contiguous().to(device)
        self.fwd_taps, rs_all, classes = conv_tap_classes(self.r, self.s, self.stride, pad)
        self.split = split
        if self.groups > 1:
            # grouped 3x3 (ResNeXt's conv2): no dense table exists.  Per slice of S channels (`grouped_slice_tables`), for the forward
            # and for every backward class: g_fwd / g_bwd[i] = (rows, frag) -- `rows` the [slices][64][K] tables ([hi | lo | hi] rows in
            # reference precision) the generic entries take slice by slice, `frag` the same values in the fragment order of
            # rart_conv3x3_grouped_* ([2][...]: hi and lo planes, in reference precision)
            assert self.cin == self.cout and self.r == 3 and self.s == 3 and pad == 1, 'grouped convolutions: 3x3, pad 1, cin == cout'
            self.gw = self.cin // self.groups
            assert self.gw in (4, 8, 16, 32, 64), 'group widths 4, 8, 16, 32, 64'
            self.slice = 64 if self.gw == 64 else 32
            self.w_fwd = None
            self.bwd = [(parity, taps, None) for parity, taps, _ in classes]
            self._g_rs = [(rs_all, False)] + [(rs, True) for _, _, rs in classes]
            tabs = [tuple(t.to(device) for t in tt) for tt in self._grouped_tables(w)]
            self.g_fwd, self.g_bwd = tabs[0], tabs[1:]
            return
        planes = _planes(w, split)

        def table(rs, transpose):
            """filter taps rs of [cout][cin][r][s] side by side.  Forward: rows = cout, k = tap * cin + c; backward to input
            (transpose): rows = cin, k = tap * cout + cout index"""
            rows = self.cin if transpose else self.cout
            return _table(lambda wb: pad_rows(torch.cat([wb[:, :, r, s].t() if transpose else wb[:, :, r, s] for r, s in rs], 1),
                                              rows_mult(rows)), planes, device)
        self.w_fwd = table(rs_all, False)
        # backward to input: list of (input parity (ph, pw) or None, taps [(dy, dx)], table or None); a stride-2 conv has one table
        # per input-parity class, over the filter taps that reach it
        self.bwd = [(parity, taps, table(rs, True) if rs else None) for parity, taps, rs in classes]

    def _grouped_tables(self, w):
        """folded fp32 weight [C][gw][3][3] -> [(rows, frag)] for the forward, then for every backward class"""
        import torch
        S, out = self.slice, []
        for rs, transpose in self._g_rs:
            pl = [grouped_slice_tables(p, rs, transpose, S) for p in _planes(w, self.split)]           # [slices][S][K], bf16-exact fp32
            rows = [torch.nn.functional.pad(p, (0, 0, 0, 64 - S)) for p in pl]                         # rows padded to the GEMM tile
            rows = _bf16(torch.cat(rows + rows[:1], 2) if len(rows) == 2 else rows[0])
            frag = [grouped_frag(p) for p in pl]
            out.append((rows, _bf16(torch.stack(frag) if len(frag) == 2 else frag[0])))
        return out

    def refold_grouped(self, w):
        """re-derive the grouped tables in place from the folded fp32 weight w (on the tables' device)"""
        for (rows, frag), (nr, nf) in zip([self.g_fwd] + list(self.g_bwd), self._grouped_tables(w)):
            rows.copy_(nr)
            frag.copy_(nf)


def grouped_slice_tables(w, rs, transpose, S):
    """Grouped weight w [C][gw][r][s] (C in = C out, groups of gw channels) -> the dense per-slice tables [C / S][S][len(rs) * S] over the
    filter taps rs: slice i covers channels i S .. i S + S - 1, which hold whole groups, so it reads only itself.  Row o, column
    t * S + c = w[i S + o][c % gw][rs[t]] where c and o lie in the same group, exactly zero elsewhere; transpose (backward to the
    input): row c, column t * S + o."""
    import torch
    C, gw, r, s = w.shape
    ns = C // S
    assert C % S == 0 and S % gw == 0
    dense = w.new_zeros(ns, S, S // gw, gw, r, s)
    o = torch.arange(S, device=w.device)
    dense[:, o, o // gw] = w.reshape(ns, S, gw, r, s)
    dense = dense.reshape(ns, S, S, r, s)                      # [slice][out][in][r][s]
    return torch.cat([dense[:, :, :, a, b].transpose(1, 2) if transpose else dense[:, :, :, a, b] for a, b in rs], 2).contiguous()


def grouped_frag(t):
    """slice tables [slices][S][K] -> the fragment order of rart_conv3x3_grouped_*: [slices][K / 16][S / 32][64 lanes][8], lane l of
    fragment (st, j) = T[j * 32 + (l & 31)][st * 16 + (l >> 5) * 8 ..]"""
    ns, S, K = t.shape
    return t.reshape(ns, S // 32, 32, K // 16, 2, 8).permute(0, 3, 1, 4, 2, 5).contiguous().view(-1)


class ResNet50Engine(EngineBase):
    """Hand-written HIP eval engine for robustart_amd.model.resnet_torch.ResNet, in one of two precisions: one launch chain
    (stem -> 16 bottlenecks -> average pool -> classifier, and back) that forks on `self.x3` only where the library entry, the
    tensor form or the fused block kernels of a precision differ.  Tables and buffers exist in the engine's precision only."""

    def __init__(self, model, device='cuda', precision='bf16'):
        """precision: 'bf16' -- bf16 storage, fp32 accumulation (the fast path; logits within ~3e-3 of the fp32 network);
        'bf16x3' (alias 'fp32x') -- REFERENCE PRECISION: the reference runs fp32 (adv/attack.py:20-23,
        autopgd_base.py:271-289) and the north star asks for logits within 1e-4 of it, so every activation, gradient and
        weight is a hi + lo pair of bf16 values (16 significand bits) and every contraction the three MFMA products
        hi.hi + hi.lo + lo.hi with fp32 accumulation: logits within ~1e-5 of the fp32 network's scale."""
        super().__init__(device, precision)
        torch = _lib.require_gpu()
        split = self.x3
        m = model
        assert not m.training, 'the attack / eval engine folds BatchNorm: call model.eval() first'
        dev = self.device
        self._build_stem(m.conv1, m.bn1)
        self.fused_stem_bwd = True       # False: max-pool bwd -> patches GEMM -> col2im (kept as the cross-check)
        self.sign_bit_masks = True       # False: the backward reads the bf16 activations for their ReLU sign (cross-check)
        self.halo_conv3x3 = True         # False: layer1 / layer2 3x3 convs on the generic implicit GEMM (cross-check)
        self.fused_stem_fwd = True       # False: prep_input -> row-tap GEMM -> max pool (cross-check; keeps acts['y1'])
        self.fused_bottleneck = True     # False: layer1's identity blocks as three conv launches each (cross-check)
        # identity blocks of layer2 / layer3 / layer4 on the image-resident fused kernels (bottleneck{28,14,7}_fused.hip):
        self.fused_bottleneck14 = True   # False: all of them as three conv launches each (cross-check)
        self.fused_bottleneck28 = True   # False: only layer2's
        self.fused_bottleneck7 = True    # False: only layer4's
        self.fused_bottleneck_s2 = True  # False: the stride-2 first blocks of layer2 / layer3 as four conv launches in the forward (cross-check)
        self.fused_bottleneck_s2_bwd = True   # False: their backward-to-input as seven conv launches (cross-check)
        self.small_m_fc = True           # False: the classifier head and its backward on the implicit GEMM (cross-check)
        self.pair_tile = (0, 0)
        self.fused_next_pair = True      # reference-precision mode: ... and the neighbouring block's 1x1 reduction in the same launch; False: its own launch (cross-check)
        self.fused_next_channels = (64,)  # ... for these mid-channel counts (measured at B = 256: layer1 -0.35 ms per gradient evaluation; layer2's instance sits at 256 VGPRs and loses 0.6 ms)
        # ... for 3x3 layers of these widths (layer1 = 64, layer2 = 128).  Round 6: layer2 left the list -- with the ping-pong kernels and the
        # 224-row tiles its two launches are faster than its tail kernel at B = 256 (196 workgroups per XCD on 64 resident: 3.06 passes):
        # 20.12 -> 19.98 ms per gradient evaluation, same bits (scratch/r6/tail_channels.py)
        self.fused_tail_channels = (64,)
        self.fused_tail_pair = True      # reference-precision mode: 3x3 + 1x1 expansion of a Bottleneck as one launch (conv_tail_pair.hip); False: two launches (cross-check)
        # reference-precision mode: the projection shortcut of a layer's first block as extra K steps of the launch it is added in (conv3's
        # two-source launch; layer1's tail kernel; backward of layer1's stride-1 shortcut inside conv1^T's launch) -- its 4C-channel skip pair
        # never exists in HBM.  False: its own launch, added as conv3's residual (cross-check).  The stride-2 shortcuts' BACKWARD, whose
        # gradient reaches one input-parity class in four, rides in conv1^T's class launch (`pair_class_launch` below)
        self.fused_shortcut_pair = True
        # reference-precision mode: the input-parity classes of a stride-2 backward-to-input as ONE launch (rart_gemm_pair_classes_bf16)
        # instead of one launch per class, for 3x3 convolutions of these widths; False / () : a launch per class (cross-check).  With
        # `fused_shortcut_pair` the stride-2 shortcuts' backward rides in conv1^T's class launch for shortcut inputs of
        # `class_shortcut_channels`: dx = mask(W1^T . dza) on the parities (0, 1) (1, 0) (1, 1), mask(W1^T . dza + Wds^T . dz) on (0, 0),
        # written once and never read.  Honoured only where the library serves four classes (the query is made once, here)
        self.pair_class_launch = True
        self.class_3x3_channels = (128, 256, 512)
        self.class_shortcut_channels = (256, 512, 1024)
        self.pair_classes = self.lib.rart_gemm_pair_max_classes() if split else 0
        # reference precision: the short-K wide 1x1 launches of identity blocks (the expansion with its skip pair, conv1^T with the gradient
        # as residual) on rart_expand_walk_pair (csrc/expand_walk_pair.hip): the A rows stay in registers while the workgroup walks all N
        # columns.  For these K (layer2's 128 -> 512, layer3's 256 -> 1024); honoured only for K up to what the library says (the query is made once, here).
        # Same bits as rart_gemm_pair_bf16.  False: every such launch on rart_gemm_pair_bf16 (cross-check)
        self.expand_walk_pair = True
        self.expand_walk_channels = (128, 256)
        self.expand_walk_max_k = self.lib.rart_expand_walk_pair_max_k() if split else 0
        # reference-precision mode: layer1 block 0's conv1 + bias + ReLU inside the fused stem forward (rart_engine_stem_fwd_next_pair): the
        # pooled pair is not re-read by a launch of its own.  False: its own launch (cross-check).  Same bits either way.  Per source form,
        # by its own measurement at B = 256 (profiles/first_block_folds_per_part.txt): uint8 sources 549 -> 496 us for stem + conv1; fp32
        # sources 485 -> 478 us, inside the run-to-run spread, so the fold stays off for them.  Honoured only where the library answers
        # rart_gemm_pair_max_classes (the entry came with it)
        self.fused_stem_next_pair = True
        self.fused_stem_next_sources = ('u8',)
        # grouped 3x3 (ResNeXt's conv2, either precision) on rart_conv3x3_grouped_* (csrc/conv_grouped.hip), for these group widths; False /
        # a width not listed: the same slice tables through the generic entries, one launch per slice (cross-check and A/B baseline:
        # profiles/grouped_conv_ab.py).  Measured at B = 256 on every conv2 shape of resnext50_32x4d, both directions and precisions
        # (profiles/grouped_conv_ab.json): the new kernel wins all 28 cases, 1.3 x to 14 x, so every width stays listed
        self.grouped_conv_kernel = True
        self.grouped_kernel_widths = (4, 8, 16, 32, 64)
        self.pair_gemm_kernel = True     # reference-precision mode: False = the three products as 3 x the taps of the implicit GEMM (round 3; cross-check)
        self.blocks = []
        for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
            for blk in layer:
                ds = _Conv(blk.downsample[0], blk.downsample[1], dev, split) if blk.downsample is not None else None
                self.blocks.append((_Conv(blk.conv1, blk.bn1, dev, split), _Conv(blk.conv2, blk.bn2, dev, split),
                                    _Conv(blk.conv3, blk.bn3, dev, split), ds))
        self._build_head(m.fc)
        # round 5 experiment, OFF by default: the pair GEMM's weight tables with the hi and the lo slice of a 32-deep K step side by side (one
        # 128-byte line per row and step instead of two half lines K apart).  2-5 % per K-deep launch when a shape is replayed back to back
        # (profiles/r05_pair_knockouts.txt), nothing on the whole gradient evaluation (20.61 vs 20.63 ms) and +0.9 % on the forward
        # (scratch/r5/ab_engine_x3.py): the isolated replay keeps the tables hot in L2, the network does not.  RART_PAIR_WIL=1 turns it on.
        self.pair_w_interleaved = _os.environ.get('RART_PAIR_WIL', '0') == '1'
        if not split:
            self._pack_frag_tables()
        else:
            self._pack_tail_tables()

    def _build_stem(self, conv, bn):
        """the tables of the stem `conv` + `bn` (7x7/2, 64 channels) in the engine's precision"""
        import torch
        split, dev = self.x3, self.device
        # ---- stem: 7x7/2 conv on the padded 4-channel hi/lo image; a "tap" = one filter row, 8 px x 4 ch
        st = _Conv(conv, bn, dev, split)
        self.stem = st
        pl = _planes(st.w_folded, split)                                  # [64][3][7][7]
        # stem backward: patches[(r*7+s)*3+c] = sum_k dz[k] * W[k][c][r][s]; 147 rows zero-padded to the tile
        self.stem_patch_cols = 152                                        # 147 rounded up to 8
        self.stem_wd = _table(lambda p: pad_rows(p.permute(2, 3, 1, 0).reshape(147, 64), rows_mult(self.stem_patch_cols)), pl, dev)
        if not split:
            self.stem_w = _table(lambda p: stem_rows(p).repeat(1, 2), pl, dev)     # the image's hi taps then its lo taps
            self.stem_wt = self._stem_bwd_table(pl[0]).to(dev)            # fused stem backward (stem_fused.hip)
        else:
            self.stem_w = _table(stem_rows, pl, dev)                     # x_hi.w_hi, x_hi.w_lo, x_lo.w_hi row taps
            self.stem_w_pair = _bf16(torch.stack([stem_rows(p) for p in pl])).to(dev)     # fused pair stem forward (stem_pair.hip): [2][64][224]
            self.stem_wt_pair = pair(self._stem_bwd_table(st.w_folded, dtype=torch.float32)).to(dev)     # fused pair stem backward

    def _build_head(self, fc):
        """the tables of the classifier `fc` in the engine's precision"""
        import torch
        split, dev = self.x3, self.device
        # ---- classifier: forward table [1024][2048], backward-to-input table [2048][1024] ([hi | lo | hi] rows in reference precision)
        wfc = fc.weight.detach().float()
        self.n_classes, self.fc_in = wfc.shape
        # (class counts that are no multiple of 8 -- small test heads: the forward launch writes n_cols8 columns, the bias is a view into a
        # vector padded with zeros to that length, and K of the backward is padded to the 64-deep step of rart_gemm_small_m_bf16)
        self.n_cols8 = (self.n_classes + 7) // 8 * 8
        fc_b = torch.zeros(self.n_cols8, dtype=torch.float32)
        fc_b[:self.n_classes] = fc.bias.detach().float()
        self.fc_b = fc_b.to(dev)[:self.n_classes]
        self.fc_kpad = (self.n_classes + 63) // 64 * 64                   # 1024
        pl = _planes(wfc, split)
        self.fc_w = _table(lambda p: pad_rows(p, 128), pl, dev)
        self.fc_wd = _table(lambda p: pad_k(p.t(), self.fc_kpad), pl, dev)

    def _pack_tail_tables(self):
        """Reference-precision mode: the 1x1 expansion tables of rart_conv3x3_tail_pair in MFMA fragment order, as [2 (hi, lo)][rows * k]:
        element ((blk * (k / 16) + s) * 64 + h * 32 + r) * 8 + e = T[blk * 32 + r][16 s + 8 h + e].  `tail_fwd` on conv3 (rows = its
        output channels), `tail_bwd` on conv1 of an identity block (rows = its INPUT channels: the transposed table of the backward)."""
        torch = _lib.require_gpu()

        def frag(tab, rows, k):          # tab: the [rows_padded][hi | lo | hi] table of _Conv(split=True)
            out = []
            for pl in range(2):
                w = tab[:rows, pl * k:(pl + 1) * k]
                out.append(w.reshape(rows // 32, 32, k // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1))
            return torch.stack(out).contiguous()
        def frag_next(tab, rows, k):     # the neighbour's reduction [rows = C][k = 4C], fragment order by 64-wide K chunk
            out = []
            for pl in range(2):
                w = tab[:rows, pl * k:(pl + 1) * k]
                out.append(w.reshape(rows // 32, 32, k // 64, 4, 2, 8).permute(2, 0, 3, 4, 1, 5).contiguous().view(-1))
            return torch.stack(out).contiguous()
        two_sources = self.lib.rart_gemm_pair_max_sources() >= 2      # the library takes a second A source per pair launch
        for bi, (ca, cb, cc, ds) in enumerate(self.blocks):
            if self.pair_classes >= 4:
                class_tables(ca, cb, ds)
            if two_sources and ds is not None and fold_shortcut_tables(ca, cc, ds) and ds.stride == 1 and ds.cin == 64 and cc.cout == 4 * cb.cout:
                ds.tail_x = frag(ds.w_fwd, ds.cout, ds.cin)        # layer1's first block: the shortcut inside the tail kernel
            if not (cb.groups == 1 and cb.r == 3 and cb.stride == 1 and cb.pad == 1 and cb.cin == cb.cout and self.lib.rart_conv3x3_tail_pair_supported(cb.cin)):
                continue
            if cc.cin == cb.cout and cc.cout == 4 * cb.cout and cc.r == 1 and cc.stride == 1:
                cc.tail_fwd = frag(cc.w_fwd, cc.cout, cc.cin)
                if bi + 1 < len(self.blocks):        # the next block's conv1 on this block's output tile
                    na = self.blocks[bi + 1][0]
                    if na.r == 1 and na.stride == 1 and na.cin == cc.cout and na.cout == cb.cout:
                        na.next_fwd = frag_next(na.w_fwd, na.cout, na.cin)
            if ds is None and ca.cout == cb.cin and ca.cin == 4 * cb.cin and ca.r == 1 and ca.stride == 1:
                ca.tail_bwd = frag(ca.bwd[0][2], ca.cin, ca.cout)
                pc = self.blocks[bi - 1][2]          # the previous block's conv3^T on this block's input-gradient tile
                if bi > 0 and pc.r == 1 and pc.stride == 1 and pc.cout == ca.cin and pc.cin == cb.cin:
                    pc.next_bwd = frag_next(pc.bwd[0][2], pc.cin, pc.cout)

    def _pack_frag_tables(self, record=None, sums=None):
        """MFMA-fragment-ordered copies of the 3x3 tables the LDS-resident kernels (conv3x3_halo.hip, bottleneck_fused.hip)
        stream from L2: a fragment load then reads 1 KiB contiguous instead of touching 32 cache lines.
        record / sums (refold): instead of launching, append every (source table, fragment table, rows, k) job to `record` and
        every (conv3 bias, shortcut bias, summed bias) triple to `sums` -- the allocations happen either way."""
        torch = _lib.require_gpu()
        sp = _lib.stream_ptr()
        lib_pack = self.lib.rart_pack_frag_bf16

        def pack(tab, dst, rows, k):
            if record is not None:
                record.append((tab, dst, rows, k))
            else:
                _lib.check(lib_pack(_lib.ptr(tab), _lib.ptr(dst), rows, k, sp))

        def bias_sum(a, b, out):
            if sums is not None:
                sums.append((a, b, out))
            else:
                torch.add(a, b, out=out)
        for ca, cb, cc, ds in self.blocks:
            if cb.groups > 1:        # a grouped 3x3 has no dense table: none of the fused kernels takes its block
                continue
            if cb.r == 3 and cb.stride == 1 and cb.cin == cb.cout and cb.cin in (64, 128, 256, 512):
                for name, tab in (('w_fwd_frag', cb.w_fwd), ('w_bwd_frag', cb.bwd[0][2])):
                    if getattr(cb, name, None) is None:
                        setattr(cb, name, torch.empty(9 * cb.cin * cb.cin, dtype=torch.bfloat16, device=self.device))
                    pack(tab, getattr(cb, name), cb.cin, 9 * cb.cin)
            if ds is None and cb.stride == 1 and (ca.cin, ca.cout, cc.cout) in ((1024, 256, 1024), (512, 128, 512), (2048, 512, 2048)):
                # identity blocks of layer2 / layer3 / layer4 for the image-resident fused kernels: both 1x1 tables in fragment order
                for c_, rows, k in ((ca, ca.cout, ca.cin), (cc, cc.cout, cc.cin)):
                    for name, tab in (('w_fwd_frag', c_.w_fwd), ('w_bwd_frag', c_.bwd[0][2])):
                        r_, k_ = (rows, k) if name == 'w_fwd_frag' else (k, rows)
                        if getattr(c_, name, None) is None:
                            setattr(c_, name, torch.empty(rows * k, dtype=torch.bfloat16, device=self.device))
                        pack(tab, getattr(c_, name), r_, k_)
            if (ds is not None and cb.stride == 2 and cb.r == 3 and ds.stride == 2 and ds.r == 1
                    and (ca.cin, ca.cout, cc.cout) in ((256, 128, 512), (512, 256, 1024))):
                # stride-2 first block of layer2 / layer3 for the fused forward kernel (bottleneck_s2_fused.hip): all four tables in
                # fragment order, conv3 + shortcut bias
                for c_, name, rows, k in ((ca, 's2_w1', ca.cout, ca.cin), (cb, 's2_w2', cb.cout, 9 * cb.cin), (cc, 's2_w3', cc.cout, cc.cin),
                                          (ds, 's2_wd', ds.cout, ds.cin)):
                    if getattr(c_, name, None) is None:
                        setattr(c_, name, torch.empty(rows * k, dtype=torch.bfloat16, device=self.device))
                    pack(c_.w_fwd, getattr(c_, name), rows, k)
                if getattr(ds, 'bias_sum', None) is None:
                    ds.bias_sum = torch.empty_like(cc.bias)
                bias_sum(cc.bias, ds.bias, ds.bias_sum)
                # ... and the backward kernel's: transposed tables of conv3 / conv1 / the shortcut, and the four input-parity-class
                # tables of the 3x3 / 2 (1 / 2 / 2 / 4 taps) packed one by one into a single buffer
                cm = ca.cout
                for c_, name, tab, rows, k in ((cc, 's2_w3t', cc.bwd[0][2], cm, cc.cout), (ca, 's2_w1t', ca.bwd[0][2], ca.cin, cm),
                                               (ds, 's2_wdt', ds.bwd[0][2], ds.cin, ds.cout)):
                    if getattr(c_, name, None) is None:
                        setattr(c_, name, torch.empty(rows * k, dtype=torch.bfloat16, device=self.device))
                    pack(tab, getattr(c_, name), rows, k)
                if getattr(cb, 's2_w2t', None) is None:
                    cb.s2_w2t = torch.empty(9 * cm * cm, dtype=torch.bfloat16, device=self.device)
                off = 0
                for (_, taps, tab) in cb.bwd:                  # parity classes (0,0) (0,1) (1,0) (1,1)
                    pack(tab, cb.s2_w2t[off:], cm, len(taps) * cm)
                    off += len(taps) * cm * cm
                assert off == 9 * cm * cm
            if (ds is not None and ds.stride == 1 and ds.r == 1 and cb.stride == 1 and ca.cin == 64 and ca.cout == 64
                    and cc.cout == 256):
                # first block of layer1 for the fused kernel: the shortcut table in fragment order, conv3 + shortcut bias
                if getattr(ds, 'w_fwd_frag', None) is None:
                    ds.w_fwd_frag = torch.empty(ds.cout * ds.cin, dtype=torch.bfloat16, device=self.device)
                    ds.bias_sum = torch.empty_like(cc.bias)
                pack(ds.w_fwd, ds.w_fwd_frag, ds.cout, ds.cin)
                bias_sum(cc.bias, ds.bias, ds.bias_sum)

    _stem_bwd_index = {}

    @staticmethod
    def _stem_bwd_table(wb, dtype=None):
        """bf16 (or `dtype`) [16][1024] table of rart_engine_stem_bwd_fused from the folded stem weights wb [64][3][7][7]:
        row (py*2+px)*3+c, column ((dp+1)*4+(dq+1))*64+k = W[k][c][py+3-2dp][px+3-2dq] (0 outside 0..6).  One gather + one scatter
        through index tensors built once per device (the adversarial-training loop calls this every step: 147 slice assignments
        were 147 tiny launches)."""
        import torch
        key = str(wb.device)
        idx = ResNet50Engine._stem_bwd_index.get(key)
        if idx is None:
            src, dst = [], []
            for py in range(2):
                for px in range(2):
                    for dp in range(-1, 3):
                        r = py + 3 - 2 * dp
                        if not 0 <= r <= 6:
                            continue
                        for dq in range(-1, 3):
                            s_ = px + 3 - 2 * dq
                            if not 0 <= s_ <= 6:
                                continue
                            for c in range(3):
                                row, blk = (py * 2 + px) * 3 + c, (dp + 1) * 4 + (dq + 1)
                                for k in range(64):
                                    dst.append(row * 1024 + blk * 64 + k)
                                    src.append(((k * 3 + c) * 7 + r) * 7 + s_)
            idx = (torch.tensor(src, dtype=torch.long, device=wb.device), torch.tensor(dst, dtype=torch.long, device=wb.device))
            ResNet50Engine._stem_bwd_index[key] = idx
        t = torch.zeros(16 * 1024, dtype=wb.dtype, device=wb.device)
        t[idx[1]] = wb.reshape(-1)[idx[0]]
        return t.reshape(16, 1024).to(dtype or torch.bfloat16).contiguous()

    # ------------------------------------------------------------------ re-fold from the live parameters
    def refold(self, model):
        """Re-derive every table from `model`'s CURRENT parameters and running statistics, on the GPU: the adversarial-training
        loop attacks the model it is training (cifar10/code/train.py:105-111), so the attack engine is refreshed every iteration.
        Round 4: the ~480 launches this took (five torch elementwise kernels + two to five rart_pack_conv_weight_bf16 calls per
        convolution, one rart_pack_frag_bf16 per fragment-ordered copy) are a handful now -- the BatchNorm fold runs on flat
        concatenated vectors, every conv table is one job of ONE rart_pack_jobs_bf16 launch, every fragment re-order one job of a
        second; the tables are bit-identical to the constructor's (tests/test_engine_gpu.py::test_refold_...)."""
        torch = _lib.require_gpu()
        if self.precision != 'bf16':
            raise NotImplementedError('refold() serves the adversarial-training loop, which attacks on the bf16 engine; build a '
                                      'new ResNet50Engine(model, precision=%r) from the updated weights instead' % self.precision)
        lib, sp = self.lib, _lib.stream_ptr()
        m = model
        pairs = [(self.stem, m.conv1, m.bn1)]
        bi = 0
        for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
            for blk in layer:
                ca, cb, cc, ds = self.blocks[bi]
                pairs += [(ca, blk.conv1, blk.bn1), (cb, blk.conv2, blk.bn2), (cc, blk.conv3, blk.bn3)]
                if ds is not None:
                    pairs.append((ds, blk.downsample[0], blk.downsample[1]))
                bi += 1
        st = getattr(self, '_refold_state', None)
        key = tuple(conv.weight.data_ptr() for _, conv, _ in pairs)
        if st is None or st['key'] != key:
            st = self._build_refold_state(pairs, key)
        # ---- BatchNorm fold on flat vectors: scale = gamma * rsqrt(var + eps), bias = beta - mean * scale
        torch.cat([bn.running_var.detach() for _, _, bn in pairs], out=st['var'])
        torch.cat([bn.weight.detach() for _, _, bn in pairs], out=st['gamma'])
        torch.cat([bn.bias.detach() for _, _, bn in pairs], out=st['beta'])
        torch.cat([bn.running_mean.detach() for _, _, bn in pairs], out=st['mean'])
        torch.add(st['var'], st['eps'], out=st['scale'])
        st['scale'].rsqrt_().mul_(st['gamma'])
        torch.mul(st['mean'], st['scale'], out=st['tmp'])
        torch.sub(st['beta'], st['tmp'], out=st['bias'])        # c.bias of every layer is a view into st['bias']
        # ---- every conv table (forward + backward-to-input classes) in one launch, every fragment-ordered copy in a second
        _lib.check(lib.rart_pack_jobs_bf16(_lib.ptr(st['pack_jobs']), st['n_pack'], 48, sp))
        for w, scale, tab, c, trs, tr in st['big']:
            _lib.check(lib.rart_pack_conv_weight_bf16(w.data_ptr(), scale.data_ptr(), tab.data_ptr(), c.cout, c.cin, c.r, c.s, len(trs),
                                                      _cints([a for a, _ in trs]), _cints([b for _, b in trs]), tr, tab.shape[0], sp))
        for c, w, scale in st['grouped']:
            c.refold_grouped(w.detach() * scale.view(-1, 1, 1, 1))
        # stem extras (row-tap table, patches table, fused-backward table) and the classifier
        sc = st['scale'][:64]
        wb = (m.conv1.weight.detach() * sc.view(-1, 1, 1, 1)).to(torch.bfloat16)          # [64][3][7][7]
        wrow = stem_rows(wb)
        self.stem_w[:, :224] = wrow
        self.stem_w[:, 224:] = wrow
        self.stem_wd.zero_()
        self.stem_wd[:147] = wb.permute(2, 3, 1, 0).reshape(147, 64)
        self.stem_wt.copy_(self._stem_bwd_table(wb.float()))
        wfb = m.fc.weight.detach().to(torch.bfloat16)
        self.fc_w[:self.n_classes] = wfb
        self.fc_wd[:, :self.n_classes] = wfb.t()
        self.fc_b.copy_(m.fc.bias.detach())
        if st['n_frag']:
            _lib.check(lib.rart_pack_jobs_bf16(_lib.ptr(st['frag_jobs']), st['n_frag'], 32, sp))
        for cc_bias, ds_bias, out in st['bias_sums']:
            torch.add(cc_bias, ds_bias, out=out)

    def _build_refold_state(self, pairs, key):
        """Persistent buffers and the two device job lists of `refold` (built once per model: every pointer in them is stable --
        parameters live in the optimizer's arena, tables and flat vectors are allocated here or in the constructor)."""
        torch = _lib.require_gpu()
        dev = self.device
        n_tot = sum(c.cout for c, _, _ in pairs)
        eps = {float(bn.eps) for _, _, bn in pairs}
        assert len(eps) == 1, 'refold folds every BatchNorm with one eps'
        st = {'key': key, 'eps': eps.pop()}
        for nm in ('var', 'gamma', 'beta', 'mean', 'scale', 'tmp', 'bias'):
            st[nm] = torch.empty(n_tot, dtype=torch.float32, device=dev)
        jobs, big, grouped, off = [], [], [], 0
        for c, conv, bn in pairs:
            w = conv.weight
            assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
            old = c.bias
            c.bias = st['bias'][off:off + c.cout]           # a view: the flat fold writes every layer's bias at once
            c.bias.copy_(old)
            scale_ptr = st['scale'][off:off + c.cout].data_ptr()
            if c.groups > 1:                                # grouped tables are re-derived by `_Conv.refold_grouped`, not by pack jobs
                grouped.append((c, w, st['scale'][off:off + c.cout]))
                off += c.cout
                continue
            rs = [(r, s_) for r in range(c.r) for s_ in range(c.s)]
            todo = [(c.w_fwd, rs, 0)]
            for parity, taps, tab in c.bwd:
                if tab is not None:
                    prs = rs if parity is None else [(r, s_) for r, s_ in rs if (parity[0] + c.pad - r) % 2 == 0 and (parity[1] + c.pad - s_) % 2 == 0]
                    todo.append((tab, prs, 1))
            for tab, trs, tr in todo:
                if len(trs) <= 16:
                    jobs.append(self._pack_job(w, scale_ptr, tab, c, trs, tr))
                else:                                       # the 7 x 7 stem's generic tables (49 taps): single launches, as before
                    big.append((w, st['scale'][off:off + c.cout], tab, c, trs, tr))
            off += c.cout
        frag, sums = [], []
        self._pack_frag_tables(record=frag, sums=sums)
        fj = []
        for src, dst, rows, k in frag:
            j = _lib.PackJob()
            j.kind, j.rows, j.k, j.src16, j.out = 1, rows, k, src.data_ptr(), dst.data_ptr()
            fj.append(j)
        st['pack_jobs'], st['n_pack'] = self._upload_jobs(jobs), len(jobs)
        st['frag_jobs'], st['n_frag'] = (self._upload_jobs(fj) if fj else None), len(fj)
        st['bias_sums'], st['big'], st['grouped'] = sums, big, grouped
        st['_keep'] = (jobs, fj)
        self._refold_state = st
        return st

    @staticmethod
    def _pack_job(w, scale_ptr, tab, c, rs, transpose):
        j = _lib.PackJob()
        j.kind, j.n_out, j.channels, j.r, j.s, j.n_taps, j.transpose, j.rows_padded = 0, c.cout, c.cin, c.r, c.s, len(rs), transpose, tab.shape[0]
        for i, (a, b) in enumerate(rs):
            j.tap_r[i], j.tap_s[i] = a, b
        j.weight, j.out_channel_scale, j.out = w.data_ptr(), scale_ptr, tab.data_ptr()
        return j

    def _upload_jobs(self, jobs):
        torch = _lib.require_gpu()
        arr = (_lib.PackJob * len(jobs))(*jobs)
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        return host.to(self.device)

    # ------------------------------------------------------------------ launches
    def _gemm(self, src, wgt, dst, batch, grid, src_hw, src_pix, k_per_tap, taps, n_cols, dst_hw, dst_pix,
              bias=None, res=None, mask=None, flags=0, stride=(1, 1), dst_stride=(1, 1), dst_off=(0, 0),
              tap_src_off=None, sign_out=None, pair=False, src2=None, walk=False):
        if pair and self.pair_gemm_kernel and len(taps) <= 16 and k_per_tap >= 32 and (k_per_tap & (k_per_tap - 1)) == 0:
            return self._gemm_pair(src, wgt, dst, batch, grid, src_hw, src_pix, k_per_tap, taps, n_cols, dst_hw, dst_pix, bias, res,
                                   mask, flags, stride, dst_stride, dst_off, sign_out, src2, walk)
        assert src2 is None, 'a second source is served by rart_gemm_pair_bf16 only'
        dst_pair_off = res_pair_off = 0
        if pair:
            # split-bf16 tensors [2][...] (hi plane, lo plane): the three products as 3x the taps, the lo planes of dst / res
            # by their element offsets (F_PAIR); an fp32 destination (F_OUT_F32) is a plain tensor
            assert tap_src_off is None and src.shape[0] == 2
            tap_src_off = [0] * (2 * len(taps)) + [lo_off(src)] * len(taps)
            taps = list(taps) * 3
            flags |= F_PAIR
            if not (flags & F_OUT_F32):
                dst_pair_off = lo_off(dst)
            if res is not None:
                res_pair_off = lo_off(res)
        self._launch_conv(conv_desc(src, wgt, dst, batch, grid, src_hw, src_pix, k_per_tap, taps, n_cols, dst_hw, dst_pix, bias=bias,
                                    res=res, mask=mask, sign_out=sign_out, flags=flags, stride=stride, dst_stride=dst_stride,
                                    dst_org=dst_off, tap_src_off=tap_src_off, dst_pair_off=dst_pair_off, res_pair_off=res_pair_off))

    def _gemm_pair(self, src, wgt, dst, batch, grid, src_hw, src_pix, k_per_tap, taps, n_cols, dst_hw, dst_pix, bias, res, mask, flags,
                   stride, dst_stride, dst_off, sign_out, src2=None, walk=False):
        """One convolution / product of the reference-precision mode on rart_gemm_pair_bf16 (csrc/gemm_pair.hip, conv mode): the four
        operand planes of a K step staged once, three MFMAs per fragment pair -- round 3 listed the three products as 3 x the taps of
        rart_conv_igemm_bf16, which fetched x_hi twice and ran at a quarter of this kernel's MFMA rate.  src / dst / res: pair tensors
        [2][...]; wgt: the [rows][hi | lo | hi] table of `_Conv(split=True)` (w_hi = columns 0..K, w_lo = columns K..2K, row stride 3K);
        mask: 1-bit ReLU mask of the destination; an fp32 destination (F_OUT_F32) is a plain tensor.  src2 = (pair tensor, its hw, its
        stride, elements per pixel, k2): a second source whose k2 channels follow in the rows of wgt (`_cat_k`).  walk: the caller's
        launch is one rart_expand_walk_pair serves (`_walk_ok`) -- the same descriptor goes to that entry."""
        assert src.shape[0] == 2
        k_tot = k_per_tap * len(taps) + (src2[4] if src2 is not None else 0)
        assert wgt.shape[1] == 3 * k_tot
        il = None
        if self.pair_w_interleaved:
            # per row and 32-deep K step: the hi slice then the lo slice (one 128-byte line per row and step instead of two half lines)
            il = self._w_il.get(wgt.data_ptr())
            if il is None:
                il = self._w_il[wgt.data_ptr()] = interleave_k32(wgt[:, :k_tot], wgt[:, k_tot:2 * k_tot])
        nbytes = None
        if self.profile is not None:
            # algorithmic bytes = every operand once: source pair pixels (4 B per element), destination pair (or fp32), residual pair,
            # both weight planes, 1 bit per destination element for a mask / sign tensor
            rows = batch * grid[0] * grid[1]
            nbytes = 4.0 * batch * src_hw[0] * src_hw[1] * k_per_tap + 4.0 * rows * n_cols * (2 if res is not None else 1) + 4.0 * k_tot * n_cols \
                + rows * n_cols / 8.0 * ((mask is not None) + (sign_out is not None))
            if src2 is not None:
                nbytes += 4.0 * batch * src2[1][0] * src2[1][1] * src2[4]
        d = gemm_pair_desc(src, wgt, dst, n_cols, src_pix, 3 * k_tot, dst_pix, wgt.shape[0], bias=bias, res=res, mask_bits=mask,
                           sign_out=sign_out, flags=flags & (F_RELU | F_OUT_F32), w_lo_off=k_tot, w_il=il, batch=batch,
                           grid=grid, src_hw=src_hw, stride=stride, k_per_tap=k_per_tap, taps=taps, dst_hw=dst_hw,
                           dst_stride=dst_stride, dst_org=dst_off, tile=self.pair_tile, src2=src2)
        if not walk:
            return self._launch_pair(d, nbytes)
        ev = self._prof_begin()
        _lib.check(self.lib.rart_expand_walk_pair(ctypes.byref(d), 0, 0, _lib.stream_ptr()))
        if ev is not None:
            self._prof_end(ev, 3 * 2.0 * d.M * d.N * d.K, 'gemm_pair', nbytes)

    def _walk_ok(self, k, n, c):
        """whether the 1x1 launch of conv c with K = k, N = n of an identity block goes to rart_expand_walk_pair"""
        return self.expand_walk_pair and self.pair_gemm_kernel and not self.pair_w_interleaved and self.pair_tile == (0, 0) and \
            c.r == 1 and c.s == 1 and c.stride == 1 and k in self.expand_walk_channels and k <= self.expand_walk_max_k and n >= 4 * k and n % 64 == 0

    def _classes_ok(self, tabs):
        """whether a launch with the class-ordered tables `tabs` = (table, classes) goes out as one class launch"""
        return tabs is not None and self.pair_class_launch and self.pair_classes >= len(tabs[1]) and self.pair_gemm_kernel and \
            not self.pair_w_interleaved

    def _gemm_pair_classes(self, src, tabs, dst, batch, grid, src_hw, src_pix, k_per_tap, n_cols, dst_hw, dst_pix, res=None, mask=None,
                           stride=(1, 1), dst_stride=(2, 2), src2=None):
        """The classes of tabs = (table, [(taps, k_off, dst_org)]) (`class_tables`) as one rart_gemm_pair_classes_bf16 launch: class i reads
        its taps of src and the slice of the table's rows from column k_off on, and writes the destination pixels of origin dst_org.  src2
        (as in `_gemm_pair`): a second source accumulated by class 0."""
        wgt, classes = tabs
        k_tot = wgt.shape[1] // 3
        assert src.shape[0] == 2 and k_tot == k_per_tap * sum(len(c[0]) for c in classes) + (src2[4] if src2 is not None else 0)
        nbytes = None
        if self.profile is not None:
            rows = batch * grid[0] * grid[1] * len(classes)
            nbytes = 4.0 * batch * src_hw[0] * src_hw[1] * k_per_tap + 4.0 * rows * n_cols * (2 if res is not None else 1) + 4.0 * k_tot * n_cols \
                + rows * n_cols / 8.0 * (mask is not None)
            if src2 is not None:
                nbytes += 4.0 * batch * src2[1][0] * src2[1][1] * src2[4]
        d = gemm_pair_cls_desc(src, wgt, dst, n_cols, src_pix, 3 * k_tot, dst_pix, wgt.shape[0],
                               [(taps, off, org, src2 is not None and i == 0) for i, (taps, off, org) in enumerate(classes)], res=res,
                               mask_bits=mask, w_lo_off=k_tot, batch=batch, grid=grid, src_hw=src_hw, stride=stride, k_per_tap=k_per_tap,
                               dst_hw=dst_hw, dst_stride=dst_stride, tile=self.pair_tile, src2=src2)
        self._launch_pair_classes(d, nbytes)

    def _tail(self, src, wgt, taps, tail, dst, batch, hw, c_mid, bias_mid=None, bias_out=None, res=None, mask_mid=None, mask_out=None,
              sign_mid=None, sign_out=None, relu=False, nxt=None, xsrc=None):
        """3x3 (c_mid -> c_mid) + point-wise step + 1x1 expansion (c_mid -> 4 c_mid) + skip pair + point-wise step of the
        reference-precision mode as ONE launch (csrc/conv_tail_pair.hip).  src / dst / res: pair tensors; wgt: the 3x3's
        [rows][hi | lo | hi] table; tail: `_pack_tail_tables`' [2][...] fragment-ordered 1x1 table.  nxt: the neighbouring block's 1x1
        reduction of the tile in the same launch -- dict(tab, dst, bias, mask, sign, relu).  xsrc = (x pair [2][B][h][w][64], its
        fragment-ordered table): the block's stride-1 projection shortcut as extra K steps of the 1x1 (res None, bias_out the bias sum)."""
        k_tot = 9 * c_mid
        assert src.shape[0] == 2 and wgt.shape[1] == 3 * k_tot and len(taps) == 9
        d = _lib.ConvTailDesc()
        d.a_hi, d.a_lo = src[0].data_ptr(), src[1].data_ptr()
        d.w_hi, d.w_lo = wgt.data_ptr(), wgt.data_ptr() + 2 * k_tot
        d.t_hi, d.t_lo = tail[0].data_ptr(), tail[1].data_ptr()
        d.bias_mid, d.bias_out = _lib.ptr(bias_mid), _lib.ptr(bias_out)
        d.mask_mid, d.mask_out, d.sign_mid, d.sign_out = _lib.ptr(mask_mid), _lib.ptr(mask_out), _lib.ptr(sign_mid), _lib.ptr(sign_out)
        if res is not None:
            d.res_hi, d.res_lo = res[0].data_ptr(), res[1].data_ptr()
        d.dst_hi, d.dst_lo = dst[0].data_ptr(), dst[1].data_ptr()
        d.batch, d.h, d.w, d.c_mid, d.ldw = batch, hw[0], hw[1], c_mid, 3 * k_tot
        d.relu_mid = d.relu_out = 1 if relu else 0
        for i, (dy, dx) in enumerate(taps):
            d.tap_dy[i], d.tap_dx[i] = dy, dx
        if xsrc is not None:
            assert res is None and c_mid == 64 and xsrc[0].shape[-1] == 64
            d.x_hi, d.x_lo, d.tx_hi, d.tx_lo = xsrc[0][0].data_ptr(), xsrc[0][1].data_ptr(), xsrc[1][0].data_ptr(), xsrc[1][1].data_ptr()
        if nxt is not None:
            d.n_hi, d.n_lo = nxt['tab'][0].data_ptr(), nxt['tab'][1].data_ptr()
            d.dstn_hi, d.dstn_lo = nxt['dst'][0].data_ptr(), nxt['dst'][1].data_ptr()
            d.bias_next, d.mask_next, d.sign_next = _lib.ptr(nxt.get('bias')), _lib.ptr(nxt.get('mask')), _lib.ptr(nxt.get('sign'))
            d.relu_next = 1 if nxt.get('relu') else 0
        ev = self._prof_begin()
        _lib.check(self.lib.rart_conv3x3_tail_pair(ctypes.byref(d), _lib.stream_ptr()))
        if ev is not None:
            px = batch * hw[0] * hw[1]
            nx, xs = (1 if nxt is not None else 0), (1 if xsrc is not None else 0)
            nbytes = 4.0 * px * c_mid * (1 + 4 + (4 if res is not None else 0) + nx + xs) + 4.0 * c_mid * c_mid * (9 + 4 + 4 * nx + 4 * xs)
            self._prof_end(ev, 3 * 2.0 * px * (k_tot * c_mid + (4 + 4 * nx + 4 * xs) * c_mid * c_mid), 'conv_tail_pair',
                           nbytes)   # MFMA FLOPs issued, algorithmic bytes (every operand once)

    def _fc(self, a, w, out, m, n, k, bias=None):
        """The classifier head / its backward: rart_gemm_small_m_bf16 (one workgroup per 32 x 32 tile, waves split K) instead of the
        16-workgroup implicit-GEMM launch; `out` fp32 or bf16."""
        torch = _lib.require_gpu()
        ev = self._prof_begin()
        _lib.check(self.lib.rart_gemm_small_m_bf16(_lib.ptr(a), a.shape[-1], _lib.ptr(w), w.shape[-1], _lib.ptr(bias), _lib.ptr(out),
                                                   out.shape[-1], 1 if out.dtype == torch.float32 else 0, m, n, k, _lib.stream_ptr()))
        if ev is not None:
            self._prof_end(ev, 2.0 * m * n * k, 'fc_small_m')

    @staticmethod
    def _fits32(n, hw, channels):
        """the fused / LDS-resident kernels address with 32-bit element offsets (their C entry points check n*H*W*C < 2^31): beyond
        that the engine sends the layer to the generic GEMM launches instead -- which refuse tensors above 2^30 elements themselves, so
        such a batch raises there rather than in the fused kernel's entry point"""
        return n * hw[0] * hw[1] * channels < (1 << 31)

    def _halo_ok(self, c, hw, n=1):
        return (c.groups == 1 and self._fits32(n, hw, c.cin) and self.halo_conv3x3 and c.r == 3 and c.s == 3 and c.stride == 1 and c.pad == 1
                and c.cin == c.cout and getattr(c, 'w_fwd_frag', None) is not None and self.lib.rart_conv3x3_halo_supported(c.cin, hw[0], hw[1]))

    def _halo(self, src, w, dst, B, hw, ch, taps, bias=None, mask=None, sign=None, relu=False):
        ev = self._prof_begin()
        _lib.check(self.lib.rart_conv3x3_halo_bf16(_lib.ptr(src), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(mask), _lib.ptr(sign),
                                                   _lib.ptr(dst), B, hw[0], hw[1], ch, _cints([t[0] for t in taps]),
                                                   _cints([t[1] for t in taps]), 1 if relu else 0, _lib.stream_ptr()))
        if ev is not None:
            self._prof_end(ev, 2.0 * B * hw[0] * hw[1] * 9 * ch * ch, 'halo3x3')

    def _bneck_ok(self, ca, cb, cc, ds, xhw, n=1):
        return (cb.groups == 1 and self._fits32(n, xhw, cc.cout) and self.fused_bottleneck and ds is None and cb.stride == 1 and cb.r == 3 and ca.r == 1 and cc.r == 1
                and ca.cin == cc.cout and getattr(cb, 'w_fwd_frag', None) is not None
                and self.lib.rart_bottleneck_fused_supported(cc.cout, ca.cout, xhw[0], xhw[1]))

    def _image_block_fn(self, ca, cb, cc, ds, xhw, n=1):
        """-> the C entry point of the image-resident fused kernel for this identity block (layer3: 14 x 14, then layer2: 28 x 28, then
        layer4: 7 x 7) or None."""
        if not (cb.groups == 1 and self._fits32(n, xhw, cc.cout) and self.fused_bottleneck14 and ds is None and getattr(ca, 'w_fwd_frag', None) is not None
                and getattr(cb, 'w_fwd_frag', None) is not None and getattr(cc, 'w_fwd_frag', None) is not None):
            return None
        if self.lib.rart_bottleneck14_fused_supported(cc.cout, ca.cout, xhw[0], xhw[1]):
            return self.lib.rart_bottleneck14_fused_bf16
        if self.fused_bottleneck28 and self.lib.rart_bottleneck28_fused_supported(cc.cout, ca.cout, xhw[0], xhw[1]):
            return self.lib.rart_bottleneck28_fused_bf16
        if self.fused_bottleneck7 and self.lib.rart_bottleneck7_fused_supported(cc.cout, ca.cout, xhw[0], xhw[1]):
            return self.lib.rart_bottleneck7_fused_bf16
        return None

    def _bneck_image(self, x, w1, w2, w3, b1, b2, b3, m1, m2, m3, out, B, hw, c_io, c_mid, taps, backward, fn):
        """One identity Bottleneck of layer2 / layer3 / layer4 as a single launch of the image-resident kernel `fn` of
        `_image_block_fn` (csrc/bottleneck28_fused.hip, bottleneck14_fused.hip, bottleneck7_fused.hip)."""
        ev = self._prof_begin()
        _lib.check(fn(
            _lib.ptr(x), _lib.ptr(w1), _lib.ptr(w2), _lib.ptr(w3), _lib.ptr(b1), _lib.ptr(b2), _lib.ptr(b3), _lib.ptr(m1),
            _lib.ptr(m2), _lib.ptr(m3), _lib.ptr(out), B, hw[0], hw[1], c_io, c_mid, _cints([t[0] for t in taps]),
            _cints([t[1] for t in taps]), 1 if backward else 0, _lib.stream_ptr()))
        if ev is not None:
            # 5th element: ALGORITHMIC HBM bytes of the launch -- x in, out, the weight tables once, the 1-bit sign tensors
            m_ = B * hw[0] * hw[1]
            by = 2 * m_ * c_io * 2 + (2 * c_io * c_mid + 9 * c_mid * c_mid) * 2 + sum(m_ * c // 8 for c, t in ((c_mid, m1), (c_mid, m2), (c_io, m3)) if t is not None)
            self._prof_end(ev, 2.0 * B * hw[0] * hw[1] * c_mid * (2 * c_io + 9 * c_mid), {14: 'bottleneck14', 28: 'bottleneck28', 7: 'bottleneck7'}[hw[0]],
                           by)

    def _s2_ok(self, ca, cb, cc, ds, xhw, n=1):
        return (cb.groups == 1 and self.fused_bottleneck_s2 and ds is not None and getattr(ds, 's2_wd', None) is not None
                and self._fits32(n, xhw, ca.cin) and self.lib.rart_bottleneck_s2_fwd_supported(ca.cin, ca.cout, cc.cout, xhw[0], xhw[1]))

    @staticmethod
    def _s2_flops(ca, cb, cc, ds, B, xhw):
        pin, pout = xhw[0] * xhw[1], xhw[0] * xhw[1] // 4
        return 2.0 * B * (pin * ca.cin * ca.cout + pout * (9 * cb.cin * cb.cout + cc.cin * cc.cout + ds.cin * ds.cout))

    def _bneck_s2(self, x, ca, cb, cc, ds, m1, m2, m3, out, B, xhw):
        """The stride-2 first block of layer2 / layer3, forward, as one launch (csrc/bottleneck_s2_fused.hip)."""
        ev = self._prof_begin()
        _lib.check(self.lib.rart_bottleneck_s2_fwd_bf16(
            _lib.ptr(x), _lib.ptr(ca.s2_w1), _lib.ptr(cb.s2_w2), _lib.ptr(cc.s2_w3), _lib.ptr(ds.s2_wd), _lib.ptr(ca.bias),
            _lib.ptr(cb.bias), _lib.ptr(ds.bias_sum), _lib.ptr(m1), _lib.ptr(m2), _lib.ptr(m3), _lib.ptr(out), B, xhw[0], xhw[1],
            ca.cin, ca.cout, cc.cout, _lib.stream_ptr()))
        if ev is not None:
            self._prof_end(ev, self._s2_flops(ca, cb, cc, ds, B, xhw), 'bottleneck_s2')

    def _bneck_s2_bwd(self, g, ca, cb, cc, ds, m2, m1, m0, dx, B, xhw):
        """Backward-to-input of the stride-2 first block of layer2 / layer3 as one launch (csrc/bottleneck_s2_fused.hip)."""
        ev = self._prof_begin()
        _lib.check(self.lib.rart_bottleneck_s2_bwd_bf16(
            _lib.ptr(g), _lib.ptr(cc.s2_w3t), _lib.ptr(cb.s2_w2t), _lib.ptr(ca.s2_w1t), _lib.ptr(ds.s2_wdt), _lib.ptr(m2), _lib.ptr(m1),
            _lib.ptr(m0), _lib.ptr(dx), B, xhw[0], xhw[1], ca.cin, ca.cout, cc.cout, _lib.stream_ptr()))
        if ev is not None:
            self._prof_end(ev, self._s2_flops(ca, cb, cc, ds, B, xhw), 'bottleneck_s2_bwd')

    def _first_ok(self, ca, cb, cc, ds, xhw, n=1):
        return (cb.groups == 1 and self._fits32(n, xhw, cc.cout) and self.fused_bottleneck and ds is not None and getattr(ds, 'w_fwd_frag', None) is not None
                and getattr(cb, 'w_fwd_frag', None) is not None
                and self.lib.rart_bottleneck_first_supported(ca.cin, ca.cout, cc.cout, xhw[0], xhw[1]))

    def _bneck(self, x, w1, w2, w3, b1, b2, b3, m1, m2, m3, out, B, hw, c_io, c_mid, taps, backward, w4=None, c_in=None):
        """One Bottleneck as a single launch (csrc/bottleneck_fused.hip), forward or backward-to-input; w4: the projection
        shortcut's table for the layer's first block (c_in input channels)."""
        ev = self._prof_begin()
        if w4 is not None:
            _lib.check(self.lib.rart_bottleneck_first_bf16(
                _lib.ptr(x), _lib.ptr(w1), _lib.ptr(w2), _lib.ptr(w3), _lib.ptr(w4), _lib.ptr(b1), _lib.ptr(b2), _lib.ptr(b3),
                _lib.ptr(m1), _lib.ptr(m2), _lib.ptr(m3), _lib.ptr(out), B, hw[0], hw[1], c_in, c_mid, c_io,
                _cints([t[0] for t in taps]), _cints([t[1] for t in taps]), 1 if backward else 0, _lib.stream_ptr()))
        else:
            _lib.check(self.lib.rart_bottleneck_fused_bf16(
                _lib.ptr(x), _lib.ptr(w1), _lib.ptr(w2), _lib.ptr(w3), _lib.ptr(b1), _lib.ptr(b2), _lib.ptr(b3), _lib.ptr(m1),
                _lib.ptr(m2), _lib.ptr(m3), _lib.ptr(out), B, hw[0], hw[1], c_io, c_mid, _cints([t[0] for t in taps]),
                _cints([t[1] for t in taps]), 1 if backward else 0, _lib.stream_ptr()))
        if ev is not None:
            k_all = (2 * c_io + 9 * c_mid) if w4 is None else (c_in + 9 * c_mid + c_io + c_in * c_io // c_mid)
            # 5th element: ALGORITHMIC HBM bytes of the launch -- x in (read ONCE: the residual re-read and the halo rows are
            # implementation traffic), out, the weight tables once, the 1-bit sign tensors
            m_, cin_ = B * hw[0] * hw[1], (c_io if w4 is None else c_in)
            by = m_ * (c_io + cin_) * 2 + ((c_io + cin_) * c_mid + 9 * c_mid * c_mid + (0 if w4 is None else c_in * c_io)) * 2 + \
                sum(m_ * c // 8 for c, t in ((c_mid, m1), (c_mid, m2), (c_io if not backward else cin_, m3)) if t is not None)
            self._prof_end(ev, 2.0 * B * hw[0] * hw[1] * c_mid * k_all, 'bottleneck', by)

    def _grouped_ok(self, c, src_hw, dst_hw, stride, B, mask):
        """whether a launch of the grouped 3x3 c goes to rart_conv3x3_grouped_* (a mask must be a 1-bit tensor there)"""
        torch = _lib.require_gpu()
        return (self.grouped_conv_kernel and c.gw in self.grouped_kernel_widths and (mask is None or mask.dtype == torch.uint8)
                and self._fits32(B, src_hw, c.cin) and self._fits32(B, dst_hw, c.cin)
                and self.lib.rart_conv3x3_grouped_supported(c.cin, c.gw, src_hw[0], src_hw[1], stride))

    def _grouped(self, c, tabs, taps, src, src_hw, dst, dst_hw, grid, B, pair, stride=1, dst_stride=1, dst_org=(0, 0), bias=None, mask=None,
                 sign=None, relu=False):
        """One launch of the grouped 3x3 convolution c (forward, backward at stride 1, or one input-parity class of the stride-2 backward):
        grid pixel (y, x) reads src at (y * stride + dy, x * stride + dx) per tap and writes dst at (y * dst_stride + oy, x * dst_stride +
        ox).  tabs = (rows, frag) of `_Conv`: the fragment-ordered table on rart_conv3x3_grouped_*, or (`grouped_conv_kernel` off, a
        width outside `grouped_kernel_widths`) the row tables through the generic entries, one launch per slice."""
        torch = _lib.require_gpu()
        rows, frag = tabs
        C, S = c.cin, c.slice
        if self._grouped_ok(c, src_hw, dst_hw, stride, B, mask):
            ev = self._prof_begin()
            geom = (B, src_hw[0], src_hw[1], C, c.gw, stride, grid[0], grid[1], len(taps), _cints([t[0] for t in taps]),
                    _cints([t[1] for t in taps]), dst_hw[0], dst_hw[1], dst_stride, dst_org[0], dst_org[1], 1 if relu else 0, _lib.stream_ptr())
            if pair:
                _lib.check(self.lib.rart_conv3x3_grouped_pair(_lib.ptr(src[0]), _lib.ptr(src[1]), _lib.ptr(frag[0]), _lib.ptr(frag[1]),
                                                              _lib.ptr(bias), _lib.ptr(mask), _lib.ptr(sign), _lib.ptr(dst[0]), _lib.ptr(dst[1]),
                                                              *geom))
            else:
                _lib.check(self.lib.rart_conv3x3_grouped_bf16(_lib.ptr(src), _lib.ptr(frag), _lib.ptr(bias), _lib.ptr(mask), _lib.ptr(sign),
                                                              _lib.ptr(dst), *geom))
            if ev is not None:
                # MFMA FLOPs issued (the padded slices; three products in pair form); algorithmic bytes: the source pixels once, the grid's
                # destination pixels once, 1 bit per destination element for a mask / sign tensor
                px = B * grid[0] * grid[1]
                eb = 4.0 if pair else 2.0
                self._prof_end(ev, (3 if pair else 1) * 2.0 * px * len(taps) * S * C, 'grouped3x3',
                               eb * C * (B * src_hw[0] * src_hw[1] + px) + px * C / 8.0 * ((mask is not None) + (sign is not None)))
            return
        fl = (F_RELU if relu else 0) | (F_MASK_BITS if (mask is not None and mask.dtype == torch.uint8) else 0)
        cut = (lambda t, off: t.view(2, -1)[:, off:]) if pair else (lambda t, off: t.view(-1)[off:])
        for i in range(C // S):
            off = i * S
            if mask is not None and mask.dtype != torch.uint8:
                m_i = mask.view(-1)[off:]          # (bf16 cross-check: the activation itself, same element offsets as dst)
            else:
                m_i = None if mask is None else mask.view(-1)[off // 8:]
            self._gemm(cut(src, off), rows[i], cut(dst, off), B, grid, src_hw, C, S, taps, S, dst_hw, C,
                       bias=None if bias is None else bias[off:off + S], mask=m_i, flags=fl, stride=(stride, stride),
                       dst_stride=(dst_stride, dst_stride), dst_off=dst_org, sign_out=None if sign is None else sign.view(-1)[off // 8:], pair=pair)

    def _conv_fwd(self, c, x, xhw, out, relu, res=None, sign=None, pair=False, identity=False):
        """identity: conv3 of an identity block (res = the block's input) whose conv2 is ungrouped: the launch may go to the walk entry"""
        B = x.shape[1] if pair else x.shape[0]
        oh, ow = xhw[0] // c.stride, xhw[1] // c.stride
        if c.groups > 1:
            assert res is None
            return self._grouped(c, c.g_fwd, c.fwd_taps, x, xhw, out, (oh, ow), (oh, ow), B, pair, stride=c.stride, bias=c.bias, sign=sign,
                                 relu=relu)
        if pair:
            return self._gemm(x, c.w_fwd, out, B, (oh, ow), xhw, c.cin, c.cin, c.fwd_taps, c.cout, (oh, ow), c.cout, bias=c.bias,
                              res=res, flags=F_RELU if relu else 0, stride=(c.stride, c.stride), sign_out=sign, pair=True,
                              walk=identity and self._walk_ok(c.cin, c.cout, c))
        if res is None and self._halo_ok(c, xhw, B):
            return self._halo(x, c.w_fwd_frag, out, B, xhw, c.cin, c.fwd_taps, bias=c.bias, sign=sign, relu=relu)
        self._gemm(x, c.w_fwd, out, B, (oh, ow), xhw, c.cin, c.cin, c.fwd_taps, c.cout, (oh, ow), c.cout,
                   bias=c.bias, res=res, flags=F_RELU if relu else 0, stride=(c.stride, c.stride), sign_out=sign)

    def _conv_bwd(self, c, dz, dz_hw, dx, dx_hw, res=None, mask=None, pair=False, identity=False):
        """dx = backward-to-input of conv c applied to dz (then + res, masked).  mask: the forward activation at dx's
        place (bf16) or its 1-bit sign tensor (uint8, written by the forward GEMM's sign_out).  identity: conv1 of an identity block
        (res = the gradient at the block's output)."""
        torch = _lib.require_gpu()
        B = dz.shape[1] if pair else dz.shape[0]
        fl = F_MASK_BITS if (mask is not None and mask.dtype == torch.uint8) else 0
        assert not pair or mask is None or fl, 'the split-bf16 mode reads ReLU masks as 1-bit tensors only'
        if c.groups > 1:
            assert res is None
            for (parity, taps, _), tabs in zip(c.bwd, c.g_bwd):     # stride 1: one class; stride 2: the four input-parity classes
                if parity is None:
                    self._grouped(c, tabs, taps, dz, dz_hw, dx, dx_hw, dx_hw, B, pair, mask=mask)
                else:
                    self._grouped(c, tabs, taps, dz, dz_hw, dx, dx_hw, (dx_hw[0] // 2, dx_hw[1] // 2), B, pair, mask=mask, dst_stride=2,
                                  dst_org=parity)
            return
        if not pair and res is None and (mask is None or fl) and self._halo_ok(c, dx_hw, B):
            return self._halo(dz, c.w_bwd_frag, dx, B, dx_hw, c.cin, c.bwd[0][1], mask=mask)
        if pair and c.groups == 1 and c.r == 3 and c.cin in self.class_3x3_channels and self._classes_ok(getattr(c, 'cls_bwd', None)) and \
                dx_hw[0] % 2 == 0 and dx_hw[1] % 2 == 0:
            # stride-2 3x3: the four input-parity classes (1 / 2 / 2 / 4 taps) in one grid
            return self._gemm_pair_classes(dz, c.cls_bwd, dx, B, (dx_hw[0] // 2, dx_hw[1] // 2), dz_hw, c.cout, c.cout, c.cin, dx_hw, c.cin,
                                           res=res, mask=mask)
        for parity, taps, w in c.bwd:
            if parity is None:
                self._gemm(dz, w, dx, B, dx_hw, dz_hw, c.cout, c.cout, taps, c.cin, dx_hw, c.cin, res=res, mask=mask,
                           flags=fl, pair=pair, walk=pair and identity and self._walk_ok(c.cout, c.cin, c))
            else:
                ph, pw = parity
                if not taps:
                    continue        # this input-parity class receives no gradient from a 1x1/2 conv
                self._gemm(dz, w, dx, B, (dx_hw[0] // 2, dx_hw[1] // 2), dz_hw, c.cout, c.cout, taps, c.cin, dx_hw,
                           c.cin, res=res, mask=mask, flags=fl, dst_stride=(2, 2), dst_off=(ph, pw), pair=pair)

    # ------------------------------------------------------------------ the chain: stem -> bottlenecks -> head, and back
    def _po(self, t):
        """how an activation goes to a library entry: its pointer, and in reference precision the element offset of the lo plane"""
        return (_lib.ptr(t), lo_off(t)) if self.x3 else (_lib.ptr(t),)

    def _logits(self, src, src_is_u8, mean, std):
        return self._forward(src, src_is_u8, mean, std, False)[0]

    def _forward(self, src, src_is_u8, mean, std, keep):
        """-> (logits fp32, acts).  keep: also write what the backward reads (pool argmax codes, ReLU signs); acts: per block
        'b%d' = (x, xhw, ya, yb, yc, ohw) and 'b%d_masks' = (mx, ma, mb), the ReLU masks of block input / conv1 / conv2 output."""
        if src_is_u8:
            B, H, W = src.shape[0], src.shape[1], src.shape[2]
        else:
            B, H, W = src.shape[0], src.shape[2], src.shape[3]
        assert H % 32 == 0 and W % 32 == 0, 'input height/width must be multiples of 32'
        # ReLU signs as 1-bit tensors; the bf16 chain can read the bf16 activations instead (cross-check), the pair chain cannot
        bits = keep and (self.x3 or self.sign_bit_masks)
        acts = {'in_shape': (B, H, W)}
        x, xhw, xs = self._stem_fwd(src, src_is_u8, mean, std, B, H, W, keep, bits, acts)
        pre_a = acts['stem_next']      # this block's conv1 was already computed by the previous block's launch (block 0: by the stem's)
        for bi in range(len(self.blocks)):
            x, xhw, xs, pre_a = self._block_fwd(bi, x, xhw, xs, B, keep, bits, pre_a, acts)
        acts['last'], acts['last_sign'] = (x, xhw), xs
        return self._head_fwd(x, xhw, B), acts

    def _backward(self, acts, dl, std):
        """d(loss)/d(x01) fp32 NCHW from the fp32 loss gradient dl [B][classes] and the `acts` of a keep=True forward."""
        B = acts['in_shape'][0]
        dz = self._head_bwd(acts, dl, B)
        pre_b = False            # this block's conv3^T was already computed by the launch of the block above
        for bi in range(len(self.blocks) - 1, -1, -1):       # dz = masked gradient at the block output (pre-ReLU)
            dz, pre_b = self._block_bwd(bi, dz, B, pre_b, acts)
        return self._stem_bwd(acts, dz, std)

    def _stem_fwd(self, src, src_is_u8, mean, std, B, H, W, keep, bits, acts):
        """normalise + hi/lo split + 7x7/2 conv + bias + ReLU + 3x3/2 max pool -> (pooled p1, its hw, its sign tensor)"""
        import torch
        lib, sp, x3 = self.lib, _lib.stream_ptr(), self.x3
        meanf, stdf, u8 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std), 1 if src_is_u8 else 0
        h1, w1 = H // 2, W // 2
        h2, w2 = h1 // 2, w1 // 2
        p1 = self._act('p1', (B, h2, w2, 64))
        parg = self._get('p1_argmax', (B, h2, w2, 64), torch.uint8) if keep else None
        xs = self._get('p1_sign', (B, h2, w2, 8), torch.uint8) if bits else None
        y1 = None
        ca = self.blocks[0][0] if self.blocks else None      # (an engine without Bottlenecks, DenseNetEngine, has no conv1 to fold in)
        nxt = ca is not None and self.fused_stem_fwd and x3 and self.fused_stem_next_pair and ('u8' if src_is_u8 else 'f32') in self.fused_stem_next_sources and \
            self.pair_classes >= 4 and self.pair_gemm_kernel and ca.r == 1 and ca.stride == 1 and ca.cin == 64 and ca.cout == 64
        acts['stem_next'] = bool(nxt)        # block 0 starts with its conv1 done
        if nxt:                               # ... with layer1 block 0's conv1 + ReLU on the pooled tile
            ya = self._act('b0_a', (B, h2, w2, 64))
            sa = self._get('b0_a_sign', (B, h2, w2, 8), torch.uint8) if bits else None
            ev = self._prof_begin()
            _lib.check(lib.rart_engine_stem_fwd_next_pair(_lib.ptr(src), u8, _lib.ptr(self.stem_w_pair[0]), _lib.ptr(self.stem_w_pair[1]),
                                                          _lib.ptr(self.stem.bias), *self._hl(p1), _lib.ptr(parg), _lib.ptr(xs),
                                                          ctypes.c_void_p(ca.w_fwd.data_ptr()), ctypes.c_void_p(ca.w_fwd.data_ptr() + 2 * 64),
                                                          ca.w_fwd.shape[1], _lib.ptr(ca.bias), *self._hl(ya), _lib.ptr(sa), B, H, W,
                                                          meanf, stdf, sp))
            if ev is not None:   # the stem's products + 3 x 64 x 64 per pooled position; bytes: image + pooled pair + conv1's output pair
                self._prof_end(ev, 3 * 2.0 * B * (h1 * w1 * 224 + h2 * w2 * 64) * 64, 'stem_pair',
                               B * H * W * 3 * (1 if src_is_u8 else 4) + 8.0 * B * h2 * w2 * 64)
        elif self.fused_stem_fwd and x3:      # one persistent kernel (stem_pair.hip)
            ev = self._prof_begin()
            _lib.check(lib.rart_engine_stem_fwd_fused_pair(_lib.ptr(src), u8, _lib.ptr(self.stem_w_pair[0]), _lib.ptr(self.stem_w_pair[1]),
                                                           _lib.ptr(self.stem.bias), *self._hl(p1), _lib.ptr(parg), _lib.ptr(xs), B, H, W,
                                                           meanf, stdf, sp))
            if ev is not None:   # issued: 3 products x (7 row taps x 32 = 224-deep K) x 64 channels per stem output; bytes: the image once + the pooled pair
                self._prof_end(ev, 3 * 2.0 * B * h1 * w1 * 224 * 64, 'stem_pair', B * H * W * 3 * (1 if src_is_u8 else 4) + 4.0 * B * h2 * w2 * 64)
        elif self.fused_stem_fwd:             # one persistent kernel (stem_fused.hip)
            _lib.check(lib.rart_engine_stem_fwd_fused(_lib.ptr(src), u8, _lib.ptr(self.stem_w), self.stem_w.shape[1], _lib.ptr(self.stem.bias),
                                                      _lib.ptr(p1), _lib.ptr(parg), _lib.ptr(xs), B, H, W, meanf, stdf, sp))
        else:                                 # cross-check: input prep -> row-tap GEMM -> max pool
            hi = self._get('in_hi', (2, B, H + 8, W + 8, 4))
            _lib.check(lib.rart_engine_prep_input(_lib.ptr(src), u8, _lib.ptr(hi[0]), _lib.ptr(hi[1]), B, H, W, meanf, stdf, sp))
            y1 = self._act('y1', (B, h1, w1, 64))
            rows = [(r, 0) for r in range(7)]
            if x3:
                self._gemm(hi, self.stem_w, y1, B, (h1, w1), (H + 8, W + 8), 4, 32, rows, 64, (h1, w1), 64, bias=self.stem.bias,
                           flags=F_RELU, stride=(2, 2), pair=True)
            else:                             # the image pair as two taps per filter row of the [hi | hi] table
                self._gemm(hi[0], self.stem_w, y1, B, (h1, w1), (H + 8, W + 8), 4, 32, rows * 2, 64, (h1, w1), 64, bias=self.stem.bias,
                           flags=F_RELU, stride=(2, 2), tap_src_off=[0] * 7 + [lo_off(hi)] * 7)
            _lib.check((lib.rart_engine_maxpool_pair if x3 else lib.rart_engine_maxpool_keep)(
                *self._po(y1), *self._po(p1), _lib.ptr(parg), _lib.ptr(xs), B, h1, w1, 64, sp))
        acts['y1'], acts['p1'], acts['p1_argmax'] = y1, p1, parg
        return p1, (h2, w2), xs

    def _fused_block(self, ca, cb, cc, ds, xhw, B, backward):
        """-> the single-launch kernel that takes this Bottleneck in this direction, or None = conv by conv.  Reference precision:
        'tail' (conv_tail_pair.hip: the 3x3 and the 1x1 after it; the other convs keep their launches).  bf16, in this order:
        'bneck' (bottleneck_fused.hip), the C entry of an image-resident kernel (14, then 28, then 7), 'first', 's2'."""
        if self.x3:
            c = ca if backward else cc       # the 1x1 of the launch; a block with a tail table has a stride-1 C -> C 3x3 (ohw = xhw)
            return 'tail' if (cb.groups == 1 and self.fused_tail_pair and cb.cin in self.fused_tail_channels
                              and getattr(c, 'tail_bwd' if backward else 'tail_fwd', None) is not None
                              and self._fits32(B, xhw, c.cin if backward else c.cout)) else None
        if self._bneck_ok(ca, cb, cc, ds, xhw, B):
            return 'bneck'
        fn = self._image_block_fn(ca, cb, cc, ds, xhw, B)
        if fn is not None:
            return fn
        if self._first_ok(ca, cb, cc, ds, xhw, B):
            return 'first'
        if (not backward or (self.fused_bottleneck_s2_bwd and getattr(cb, 's2_w2t', None) is not None)) and self._s2_ok(ca, cb, cc, ds, xhw, B):
            return 's2'
        return None

    def _block_fwd(self, bi, x, xhw, xs, B, keep, bits, pre_a, acts):
        """Bottleneck bi -> (output, its hw, its sign tensor, whether the launch also ran conv1 of block bi + 1)"""
        import torch
        x3 = self.x3
        get, lead = self._get, ((2, B) if x3 else (B,))       # an activation: bf16 [B][h][w][c], or the pair [2][B][h][w][c]
        ca, cb, cc, ds = self.blocks[bi]
        ohw = (xhw[0] // cb.stride, xhw[1] // cb.stride)
        sa = get('b%d_a_sign' % bi, (B, xhw[0], xhw[1], ca.cout // 8), torch.uint8) if bits else None
        sb = get('b%d_b_sign' % bi, (B, ohw[0], ohw[1], cb.cout // 8), torch.uint8) if bits else None
        sc = get('b%d_c_sign' % bi, (B, ohw[0], ohw[1], cc.cout // 8), torch.uint8) if bits else None
        yc = get('b%d_c' % bi, lead + (ohw[0], ohw[1], cc.cout))
        ya = yb = None           # a fused kernel keeps its intermediates on chip: allocated only where a launch writes them
        nxt = None
        # the fused kernels emit ReLU signs as 1-bit tensors only
        kind = self._fused_block(ca, cb, cc, ds, xhw, B, False) if (bits or not keep) else None
        if kind == 'bneck':
            self._bneck(x, ca.w_fwd, cb.w_fwd_frag, cc.w_fwd, ca.bias, cb.bias, cc.bias, sa, sb, sc, yc, B, xhw, cc.cout, ca.cout,
                        cb.fwd_taps, False)
        elif kind == 'first':
            self._bneck(x, ca.w_fwd, cb.w_fwd_frag, cc.w_fwd, ca.bias, cb.bias, ds.bias_sum, sa, sb, sc, yc, B, xhw, cc.cout, ca.cout,
                        cb.fwd_taps, False, w4=ds.w_fwd_frag, c_in=ca.cin)
        elif kind == 's2':
            self._bneck_s2(x, ca, cb, cc, ds, sa, sb, sc, yc, B, xhw)
        elif kind not in (None, 'tail'):
            self._bneck_image(x, ca.w_fwd_frag, cb.w_fwd_frag, cc.w_fwd_frag, ca.bias, cb.bias, cc.bias, sa, sb, sc, yc, B, xhw, cc.cout,
                              ca.cout, cb.fwd_taps, False, kind)
        else:
            ya = get('b%d_a' % bi, lead + (xhw[0], xhw[1], ca.cout))
            if not pre_a:
                self._conv_fwd(ca, x, xhw, ya, True, sign=sa, pair=x3)
            # reference precision: the projection shortcut rides in the launch it is added in (`fused_shortcut_pair`)
            fold = x3 and ds is not None and self.fused_shortcut_pair and self.pair_gemm_kernel and \
                getattr(ds, 'tail_x' if kind == 'tail' else 'w_cat', None) is not None
            if x3:               # (the pair chain launches the projection shortcut before conv2, the bf16 chain after it)
                sk = x if ds is None else (None if fold else self._shortcut_fwd(bi, ds, x, xhw, ohw, B))
            if kind == 'tail':   # conv2 + relu + conv3 + skip + relu in one launch: the 3x3's output never exists in HBM
                na = self.blocks[bi + 1][0] if bi + 1 < len(self.blocks) else None
                if self.fused_next_pair and cb.groups == 1 and na is not None and getattr(na, 'next_fwd', None) is not None and cb.cout in self.fused_next_channels:
                    # ... and the next block's conv1 + relu on the output tile: that block's own read of this output disappears
                    nxt = dict(tab=na.next_fwd, bias=na.bias, relu=True, dst=get('b%d_a' % (bi + 1), lead + (ohw[0], ohw[1], na.cout)),
                               sign=get('b%d_a_sign' % (bi + 1), (B, ohw[0], ohw[1], na.cout // 8), torch.uint8) if keep else None)
                self._tail(ya, cb.w_fwd, cb.fwd_taps, cc.tail_fwd, yc, B, ohw, cb.cout, bias_mid=cb.bias,
                           bias_out=ds.bias_cat if fold else cc.bias, res=sk, sign_mid=sb, sign_out=sc, relu=True, nxt=nxt,
                           xsrc=(x, ds.tail_x) if fold else None)
            else:
                yb = get('b%d_b' % bi, lead + (ohw[0], ohw[1], cb.cout))
                self._conv_fwd(cb, ya, xhw, yb, True, sign=sb, pair=x3)
                if not x3:
                    sk = x if ds is None else self._shortcut_fwd(bi, ds, x, xhw, ohw, B)
                if fold:         # conv3 and the shortcut as one two-source launch: K = cc.cin + ds.cin
                    self._gemm(yb, ds.w_cat, yc, B, ohw, ohw, cc.cin, cc.cin, cc.fwd_taps, cc.cout, ohw, cc.cout, bias=ds.bias_cat,
                               flags=F_RELU, sign_out=sc, pair=True, src2=(x, xhw, (ds.stride, ds.stride), ca.cin, ds.cin))
                else:
                    self._conv_fwd(cc, yb, ohw, yc, True, res=sk, sign=sc, pair=x3, identity=ds is None and cb.groups == 1)
        acts['b%d' % bi] = (x, xhw, ya, yb, yc, ohw)
        # the backward pass needs the activations only for their ReLU sign: the 1-bit tensors, or with `sign_bit_masks` off (bf16
        # cross-check) the activations themselves
        acts['b%d_masks' % bi] = (xs, sa, sb) if (bits or x3 or kind is not None) else (x, ya, yb)
        return yc, ohw, sc, nxt is not None

    def _shortcut_fwd(self, bi, ds, x, xhw, ohw, B):
        """-> the projection shortcut ds of Bottleneck bi's input"""
        sk = self._act('b%d_ds' % bi, (B, ohw[0], ohw[1], ds.cout))
        self._conv_fwd(ds, x, xhw, sk, False, pair=self.x3)
        return sk

    def _head_fwd(self, x, xhw, B):
        """average pool + classifier -> logits fp32"""
        torch = _lib.require_gpu()
        lib, x3 = self.lib, self.x3
        pooled = self._act('pooled', (B, self.fc_in))
        _lib.check((lib.rart_engine_avgpool_pair if x3 else lib.rart_engine_avgpool)(
            *self._po(x), *self._po(pooled), B, xhw[0] * xhw[1], self.fc_in, _lib.stream_ptr()))
        logits = torch.empty(B, self.n_cols8, dtype=torch.float32, device=self.device)
        if self.small_m_fc and not x3:
            self._fc(pooled, self.fc_w, logits, B, self.n_classes, self.fc_in, bias=self.fc_b)
        else:
            self._gemm(pooled, self.fc_w, logits, B, (1, 1), (1, 1), self.fc_in, self.fc_in, [(0, 0)], self.n_cols8,
                       (1, 1), self.n_cols8, bias=self.fc_b, flags=F_OUT_F32, pair=x3)
        return logits if self.n_cols8 == self.n_classes else logits[:, :self.n_classes].contiguous()

    def _head_bwd(self, acts, dl, B):
        """classifier^T + average-pool backward with the last block's ReLU mask -> gradient at the last block's output"""
        lib, x3 = self.lib, self.x3
        # dpool[B][2048] = dlogits[B][1024 padded] . Wfc
        dlb = self._dlogits_rows(dl, 'g_dl', B, self.fc_kpad)
        dpool = self._act('dpool', (B, self.fc_in))
        if self.small_m_fc and not x3:
            self._fc(dlb, self.fc_wd, dpool, B, self.fc_in, self.fc_kpad)
        else:
            self._gemm(dlb, self.fc_wd, dpool, B, (1, 1), (1, 1), self.fc_kpad, self.fc_kpad, [(0, 0)], self.fc_in, (1, 1),
                       self.fc_in, pair=x3)
        xl, xlhw = acts['last']
        dz = self._get('g_out_%d' % (len(self.blocks) - 1), tuple(xl.shape))
        # the ReLU mask: the pair entry reads the sign tensor, the bf16 entry the activation itself
        _lib.check((lib.rart_engine_avgpool_bwd_pair if x3 else lib.rart_engine_avgpool_bwd)(
            _lib.ptr(acts['last_sign'] if x3 else xl), *self._po(dpool), *self._po(dz), B, xlhw[0] * xlhw[1], self.fc_in, _lib.stream_ptr()))
        return dz

    def _block_bwd(self, bi, dz, B, pre_b, acts):
        """backward-to-input of Bottleneck bi -> (gradient at its input, whether the launch also ran conv3^T of block bi - 1)"""
        import torch
        x3 = self.x3
        get, lead = self._get, ((2, B) if x3 else (B,))
        ca, cb, cc, ds = self.blocks[bi]
        x, xhw, ya, yb, yc, ohw = acts['b%d' % bi]
        mx, ma, mb = acts['b%d_masks' % bi]
        dx = get('g_out_%d' % (bi - 1), tuple(x.shape))
        # the fused kernels read ReLU masks as 1-bit tensors only
        if x3:
            bits = ma is not None and mx is not None
        else:
            bits = ma is not None and ma.dtype == torch.uint8 and mb is not None
        kind = self._fused_block(ca, cb, cc, ds, xhw, B, True) if bits else None
        if kind == 'bneck':
            self._bneck(dz, cc.bwd[0][2], cb.w_bwd_frag, ca.bwd[0][2], None, None, None, mb, ma, mx, dx, B, xhw, cc.cout, ca.cout,
                        cb.bwd[0][1], True)
        elif kind == 'first':
            self._bneck(dz, cc.bwd[0][2], cb.w_bwd_frag, ds.bwd[0][2], None, None, None, mb, ma, mx, dx, B, xhw, cc.cout, ca.cout,
                        cb.bwd[0][1], True, w4=ca.bwd[0][2], c_in=ca.cin)
        elif kind == 's2':
            self._bneck_s2_bwd(dz, ca, cb, cc, ds, mb, ma, mx, dx, B, xhw)
        elif kind not in (None, 'tail'):
            self._bneck_image(dz, cc.w_bwd_frag, cb.w_bwd_frag, ca.w_bwd_frag, None, None, None, mb, ma, mx, dx, B, xhw, cc.cout, ca.cout,
                              cb.bwd[0][1], True, kind)
        else:
            # (shapes from the layer geometry: a fused forward never materialises ya / yb.)  The pair chain alternates two buffers:
            # the launch of the block above may have written this block's while its own was live
            dzb = get('g_b%d' % (bi & 1) if x3 else 'g_b', lead + (ohw[0], ohw[1], cb.cout))
            if not pre_b:
                self._conv_bwd(cc, dz, ohw, dzb, ohw, mask=mb, pair=x3)
            if kind == 'tail':   # conv2^T + mask + conv1^T + identity-skip gradient + mask in one launch
                nxt = None
                pc = self.blocks[bi - 1][2] if bi > 0 else None
                if self.fused_next_pair and cb.groups == 1 and pc is not None and getattr(pc, 'next_bwd', None) is not None and cb.cin in self.fused_next_channels:
                    # ... and the previous block's conv3^T + mask on the input-gradient tile, when that block kept a mask
                    mask = acts['b%d_masks' % (bi - 1)][2]
                    if mask is not None:
                        nxt = dict(tab=pc.next_bwd, mask=mask, dst=get('g_b%d' % ((bi - 1) & 1), lead + (xhw[0], xhw[1], pc.cin)))
                self._tail(dzb, cb.bwd[0][2], cb.bwd[0][1], ca.tail_bwd, dx, B, xhw, cb.cin, res=dz, mask_mid=ma, mask_out=mx, nxt=nxt)
                return dx, nxt is not None
            dza = get('g_a', lead + (xhw[0], xhw[1], ca.cout))
            self._conv_bwd(cb, dzb, ohw, dza, xhw, mask=ma, pair=x3)
            if ds is None:
                self._conv_bwd(ca, dza, xhw, dx, xhw, res=dz, mask=mx, pair=x3, identity=cb.groups == 1)     # identity skip
            elif x3 and self.fused_shortcut_pair and self.pair_gemm_kernel and getattr(ds, 'w_cat_bwd', None) is not None:
                # stride-1 projection skip (layer1's first block): conv1^T and the shortcut^T as one two-source launch, dx written once
                self._gemm(dza, ds.w_cat_bwd, dx, B, xhw, xhw, ca.cout, ca.cout, ca.bwd[0][1], ca.cin, xhw, ca.cin, mask=mx,
                           flags=F_MASK_BITS, pair=True, src2=(dz, ohw, (1, 1), ds.cout, ds.cout))
            elif x3 and self.fused_shortcut_pair and ds.cin in self.class_shortcut_channels and self._classes_ok(getattr(ds, 'cls_bwd', None)) \
                    and xhw[0] % 2 == 0 and xhw[1] % 2 == 0:
                # stride-2 projection skip: conv1^T per input parity in one class launch, the shortcut^T as the second source of the class
                # (0, 0) -- the only one its gradient reaches -- so dx is written once and never read
                self._gemm_pair_classes(dza, ds.cls_bwd, dx, B, ohw, xhw, ca.cout, ca.cout, ca.cin, xhw, ca.cin, mask=mx, stride=(2, 2),
                                        src2=(dz, ohw, (1, 1), ds.cout, ds.cout))
            else:
                self._conv_bwd(ca, dza, xhw, dx, xhw, mask=mx, pair=x3)
                self._conv_bwd(ds, dz, ohw, dx, xhw, res=dx, mask=mx, pair=x3)             # accumulate the projection skip
        return dx, False

    def _stem_bwd(self, acts, dz, std):
        """max-pool backward + ReLU mask + transposed 7x7/2 conv -> d(loss)/d(x01) fp32 NCHW"""
        torch = _lib.require_gpu()
        lib, sp, x3 = self.lib, _lib.stream_ptr(), self.x3
        B, H, W = acts['in_shape']
        grad = torch.empty(B, 3, H, W, dtype=torch.float32, device=self.device)
        stdf = (ctypes.c_float * 3)(*std)
        parg = acts['p1_argmax']
        if self.fused_stem_bwd and x3:        # one kernel (stem_pair.hip)
            ev = self._prof_begin()
            _lib.check(lib.rart_engine_stem_bwd_fused_pair(*self._hl(dz), _lib.ptr(parg), *self._hl(self.stem_wt_pair), _lib.ptr(grad),
                                                           B, H, W, stdf, sp))
            if ev is not None:
                # issued: M = stem-output positions, K = 16 taps x 64 channels, N = 16 (4 pixel parities x 3 colours, padded); bytes: pooled
                # gradient pair + argmax codes + the fp32 image gradient
                self._prof_end(ev, 3 * 2.0 * B * (H // 2) * (W // 2) * 16 * 64 * 16, 'stem_pair', 4.0 * B * (H // 4) * (W // 4) * 64 * 1.25 + 4.0 * B * H * W * 3)
            return grad
        if self.fused_stem_bwd:               # one kernel (stem_fused.hip)
            _lib.check(lib.rart_engine_stem_bwd_fused(_lib.ptr(dz), _lib.ptr(parg), _lib.ptr(self.stem_wt), _lib.ptr(grad), B, H, W, stdf, sp))
            return grad
        # cross-check: max-pool backward (+ ReLU mask), patches GEMM, col2im to the fp32 image (bf16 patches, fp32 from pairs)
        y1 = acts['y1']          # the bf16 entry reads the stem output for its ReLU mask, the pair entry the argmax codes alone
        assert x3 or y1 is not None, 'the unfused stem backward needs the stem output: set fused_stem_fwd = False as well'
        h1, w1 = H // 2, W // 2
        dz1 = self._act('g_y1', (B, h1, w1, 64))
        if x3:
            _lib.check(lib.rart_engine_maxpool_bwd_pair(_lib.ptr(parg), *self._po(dz), *self._po(dz1), B, h1, w1, 64, sp))
        else:
            _lib.check(lib.rart_engine_maxpool_bwd(_lib.ptr(y1), _lib.ptr(parg), _lib.ptr(dz), _lib.ptr(dz1), B, h1, w1, 64, sp))
        pc = self.stem_patch_cols
        patches = self._get('patches', (B, h1, w1, pc), torch.float32 if x3 else torch.bfloat16)
        self._gemm(dz1, self.stem_wd, patches, B, (h1, w1), (h1, w1), 64, 64, [(0, 0)], pc, (h1, w1), pc, flags=F_OUT_F32 if x3 else 0,
                   pair=x3)
        _lib.check((lib.rart_engine_stem_col2im_f32 if x3 else lib.rart_engine_stem_col2im)(_lib.ptr(patches), _lib.ptr(grad), B, H, W, pc,
                                                                                             stdf, sp))
        return grad

    # ------------------------------------------------------------------ forward + backward to the input
    def forward_backward(self, x01, mean, std, y, kind, y_target=None, scale=1.0):
        """-> (logits fp32, loss_indiv, d(sum_i scale*loss_i)/dx01 fp32 NCHW, pred int32)."""
        from ..noise.adv import logit_loss
        logits, acts = self._forward(x01.detach().float().contiguous(), False, mean, std, keep=True)
        self.last_acts = acts            # exposed for the parity tests (ReLU masks of this forward)
        loss, dl, pred = logit_loss(logits, y, kind, y_target, scale)
        self.last_dlogits = dl
        return logits, loss, self._backward(acts, dl, std), pred


def make_engine(torch_model, device='cuda', precision='bf16'):
    """HIP engine for a model from robustart_amd.model.get_model: ResNet-50 and its Bottleneck family (ResNet-101/152, Wide-ResNet,
    ResNeXt: the same ResNet50Engine, which reads block counts, widths and groups from the module), ViT-B/16, ConvNeXt-B, ConvNeXt-V2-B (a ConvNeXt
    subclass: ConvNeXtEngine runs its GRN blocks), MLP-Mixer-B/16 (MixerEngine), DenseNet-121/169/201 (DenseNetEngine) or ResNet-18/34
    (BasicResNetEngine), each with forward and
    backward-to-input (`forward_backward`) on the hand-written kernels.  precision 'bf16x3' / 'fp32x': the
    reference-precision mode (both architectures: split-bf16 pairs, three MFMA products per contraction)."""
    from .resnet_torch import ResNet
    from .vit_torch import VisionTransformer
    if isinstance(torch_model, ResNet):
        return ResNet50Engine(torch_model, device, precision)
    if isinstance(torch_model, VisionTransformer):
        from .vit_engine import ViTEngine
        return ViTEngine(torch_model, device, precision)
    from .convnext_torch import ConvNeXt
    if isinstance(torch_model, ConvNeXt):
        from .convnext_engine import ConvNeXtEngine
        return ConvNeXtEngine(torch_model, device, precision)
    from .mixer_torch import MlpMixer
    if isinstance(torch_model, MlpMixer):
        from .mixer_engine import MixerEngine
        return MixerEngine(torch_model, device, precision)
    from .densenet_torch import DenseNet
    if isinstance(torch_model, DenseNet):
        from .densenet_engine import DenseNetEngine
        return DenseNetEngine(torch_model, device, precision)
    from .resnet_basic_torch import BasicResNet
    if isinstance(torch_model, BasicResNet):
        from .basic_resnet_engine import BasicResNetEngine
        return BasicResNetEngine(torch_model, device, precision)
    raise NotImplementedError('no HIP engine for %s (the ResNet Bottleneck family / ViT-B/16 / ConvNeXt-B / ConvNeXt-V2-B / MLP-Mixer-B/16 / DenseNet / '
                              'ResNet-18/34 only)'
                              % type(torch_model).__name__)


class EngineModel:
    """Callable wrapper that carries a ResNet50Engine through the reference's `model` / `f_model` keys.

    takes_normalized=True  -> drop-in for the reference's `model` (input already normalised; used by
                               mim_linf / autoattack_linf, which apply ImageNet mean/std themselves);
    takes_normalized=False -> drop-in for a foolbox PyTorchModel(model, bounds=(0,1), preprocessing=
                               dict(mean, std, axis=-3)) -- the `f_model` of pgd_linf / pgd_l2 / fgsm."""

    def __init__(self, torch_model, takes_normalized, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                 engine=None, device='cuda', precision='bf16'):
        self.rart_engine = engine or make_engine(torch_model, device, precision)
        self.takes_normalized = takes_normalized
        self.rart_mean_std = (tuple(mean), tuple(std))
        self.rart_torch_model = torch_model          # kept so a reference-precision engine can be folded from the same weights
        self._rart_ref_engine = None

    def rart_reference_engine(self):
        """The reference-precision ('fp32x') engine of the same module, built once and cached; the engine itself when it
        already runs at that precision; None when this wrapper was given a bare engine (no module to fold from).
        FAB needs it: its boundary projections work on the logit DIFFERENCE near zero, where bf16 storage dominates
        (fab_pt.py:102-117; 34 % vs 5 % robust on the fitted network)."""
        if self.rart_engine.precision != 'bf16':
            return self.rart_engine
        if self._rart_ref_engine is None and self.rart_torch_model is not None:
            self._rart_ref_engine = make_engine(self.rart_torch_model, self.rart_engine.device, 'fp32x')
        return self._rart_ref_engine

    def rart_refold(self, torch_model=None):
        """adversarial training: refresh the bf16 engine from the live weights and drop the cached reference engine"""
        self.rart_engine.refold(torch_model or self.rart_torch_model)
        self._rart_ref_engine = None

    def __call__(self, x):
        if self.takes_normalized:
            return self.rart_engine.logits(x, (0., 0., 0.), (1., 1., 1.))
        return self.rart_engine.logits(x, *self.rart_mean_std)
