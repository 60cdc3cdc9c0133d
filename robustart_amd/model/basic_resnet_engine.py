"""Eval-mode ResNet-18 / ResNet-34 on the hand-written HIP kernels: forward and backward-to-input, both precisions.

A BasicBlock net is the stem and the head of ResNet-50 around blocks of two 3x3 convolutions, so this engine extends ResNet50Engine
(stem, head, `_gemm`, `_conv_fwd` / `_conv_bwd`, buffers, profiling hooks) and replaces the chain between stem and head.

  conv-by-conv route (`basic_block_kernel = False`; always taken in reference precision, for a block with a projection, and for a
    width outside `basic_block_widths`): conv1 with folded BatchNorm + ReLU + sign bits, the 1x1 / stride projection as its own launch,
    conv2 with folded BatchNorm + residual + ReLU + sign bits -- on rart_conv3x3_halo_bf16 where `_halo_ok` allows it, otherwise on
    rart_conv_igemm_bf16 / rart_gemm_pair_bf16.  Backward: the masked gradient at the block output through conv2^T (masked by conv1's
    signs), then conv1^T plus the skip gradient, masked by the signs of the block input (the conventions of ResNet50Engine._block_bwd);
    a stride-2 3x3 runs its backward per input-parity class (`conv_tap_classes`).
  fused route (bf16, identity blocks whose shape rart_basic_block_supported accepts): one launch of rart_basic_block_bf16
    (csrc/basic_block.hip) per direction; the intermediate never exists in HBM, only its sign bits do.
"""
from .. import _lib
from .engine import ResNet50Engine, _Conv
from .engine_base import EngineBase, check_precision, cints as _cints


def check_basic(model):
    """-> the blocks of a module BasicResNetEngine takes, layer by layer; NotImplementedError otherwise"""
    c = model.conv1
    if c.out_channels != 64 or c.kernel_size != (7, 7) or c.stride != (2, 2):
        raise NotImplementedError('BasicResNetEngine: the stem is ResNet\'s 7x7 / 2 convolution to 64 channels (got %d channels)' % c.out_channels)
    blocks = [blk for layer in (model.layer1, model.layer2, model.layer3, model.layer4) for blk in layer]
    for blk in blocks:
        for conv in (blk.conv1, blk.conv2):
            if conv.kernel_size != (3, 3) or conv.groups != 1 or conv.in_channels % 32 or conv.out_channels % 32:
                raise NotImplementedError('BasicResNetEngine: a BasicBlock is two ungrouped 3x3 convolutions of widths that are multiples of 32')
    return blocks


class BasicResNetEngine(ResNet50Engine):
    """Hand-written HIP eval engine for robustart_amd.model.resnet_basic_torch.BasicResNet, bf16 or reference precision ('fp32x')."""

    def __init__(self, model, device='cuda', precision='bf16'):
        check_precision(precision)
        assert not model.training, 'the attack / eval engine folds BatchNorm: call model.eval() first'
        blocks = check_basic(model)                  # before anything touches the GPU
        EngineBase.__init__(self, device, precision)
        torch = _lib.require_gpu()
        dev, split = self.device, self.x3
        # the switches of ResNet50Engine that the inherited stem / head / convolution launchers read
        self.fused_stem_fwd = self.fused_stem_bwd = self.sign_bit_masks = self.pair_gemm_kernel = self.halo_conv3x3 = True
        self.fused_stem_next_pair, self.fused_stem_next_sources, self.pair_classes = False, (), 0
        self.pair_tile, self.pair_w_interleaved = (0, 0), False
        self.pair_class_launch, self.class_3x3_channels = False, ()
        self.blocks = []                             # no Bottlenecks
        # identity blocks as ONE launch of rart_basic_block_bf16 per direction (bf16 only).  False: conv by conv (cross-check and A/B
        # baseline: profiles/basic_block_ab.py).  `basic_block_widths`: the widths that take the fused route by default -- a width is listed
        # only if, at B = 256 and in both directions, the fused launch's slowest group of timings is below the two launches' fastest
        # (profiles/basic_block_ab.json)
        self.basic_block_kernel = True
        self.basic_block_widths = BASIC_BLOCK_WIDTHS
        self._build_stem(model.conv1, model.bn1)
        self.basic = []
        for blk in blocks:
            ds = _Conv(blk.downsample[0], blk.downsample[1], dev, split) if blk.downsample is not None else None
            c1, c2 = _Conv(blk.conv1, blk.bn1, dev, split), _Conv(blk.conv2, blk.bn2, dev, split)
            if not split:
                for c in (c1, c2):       # fragment-ordered copies for rart_conv3x3_halo_bf16 and rart_basic_block_bf16
                    if c.stride == 1 and c.cin == c.cout and c.cin in (64, 128, 256):
                        for name, tab in (('w_fwd_frag', c.w_fwd), ('w_bwd_frag', c.bwd[0][2])):
                            frag = torch.empty(9 * c.cin * c.cin, dtype=torch.bfloat16, device=dev)
                            _lib.check(self.lib.rart_pack_frag_bf16(_lib.ptr(tab), _lib.ptr(frag), c.cin, 9 * c.cin, _lib.stream_ptr()))
                            setattr(c, name, frag)
            self.basic.append((c1, c2, ds))
        self._build_head(model.fc)
        self.small_m_fc = self.fc_in % 64 == 0       # rart_gemm_small_m_bf16 steps K by 64

    def refold(self, model):
        raise NotImplementedError('refold() serves the adversarial-training loop; the BasicBlock ResNets are evaluation only: build a new '
                                  'BasicResNetEngine(model, precision=%r) from the updated weights instead' % self.precision)

    # ------------------------------------------------------------------ the fused launch
    def _basic_ok(self, c1, c2, ds, xhw, n):
        """whether this block goes out as one rart_basic_block_bf16 launch per direction"""
        return (not self.x3 and self.basic_block_kernel and ds is None and c1.stride == 1 and c1.cin == c1.cout == c2.cout
                and c1.cin in self.basic_block_widths and getattr(c1, 'w_fwd_frag', None) is not None
                and getattr(c2, 'w_fwd_frag', None) is not None and self._fits32(n, xhw, c1.cin)
                and bool(self.lib.rart_basic_block_supported(c1.cin, xhw[0], xhw[1])))

    def _basic(self, x, w1, w2, b1, b2, m_mid, m_io, out, B, hw, ch, taps, backward):
        ev = self._prof_begin()
        _lib.check(self.lib.rart_basic_block_bf16(_lib.ptr(x), _lib.ptr(w1), _lib.ptr(w2), _lib.ptr(b1), _lib.ptr(b2), _lib.ptr(m_mid),
                                                  _lib.ptr(m_io), _lib.ptr(out), B, hw[0], hw[1], ch, _cints([t[0] for t in taps]),
                                                  _cints([t[1] for t in taps]), 1 if backward else 0, _lib.stream_ptr()))
        if ev is not None:
            # FLOPs of the two convolutions (the halo recompute is implementation work); algorithmic bytes: x, out, both tables, the 1-bit
            # tensors once
            m_ = B * hw[0] * hw[1]
            self._prof_end(ev, 2.0 * m_ * 2 * 9 * ch * ch, 'basic_block',
                           2.0 * 2 * m_ * ch + 2.0 * 2 * 9 * ch * ch + m_ * ch / 8.0 * ((m_mid is not None) + (m_io is not None)))

    # ------------------------------------------------------------------ the chain
    def _forward(self, src, src_is_u8, mean, std, keep):
        """-> (logits fp32, acts).  keep: also write what the backward reads: the pool's argmax codes and, per block, 'b%d' = (input shape,
        input hw, output hw, sign bits of the block input, sign bits of the intermediate)."""
        import torch
        if src_is_u8:
            B, H, W = src.shape[0], src.shape[1], src.shape[2]
        else:
            B, H, W = src.shape[0], src.shape[2], src.shape[3]
        assert H % 32 == 0 and W % 32 == 0, 'input height/width must be multiples of 32'
        x3, get = self.x3, self._get
        acts = {'in_shape': (B, H, W)}
        x, xhw, xs = self._stem_fwd(src, src_is_u8, mean, std, B, H, W, keep, keep, acts)
        for bi, (c1, c2, ds) in enumerate(self.basic):
            ohw = (xhw[0] // c1.stride, xhw[1] // c1.stride)
            sa = get('b%d_a_sign' % bi, (B, ohw[0], ohw[1], c1.cout // 8), torch.uint8) if keep else None
            so = get('b%d_sign' % bi, (B, ohw[0], ohw[1], c2.cout // 8), torch.uint8) if keep else None
            y = self._act('b%d_out' % bi, (B, ohw[0], ohw[1], c2.cout))
            if self._basic_ok(c1, c2, ds, xhw, B):
                self._basic(x, c1.w_fwd_frag, c2.w_fwd_frag, c1.bias, c2.bias, sa, so, y, B, xhw, c1.cin, c1.fwd_taps, False)
            else:
                ya = self._act('b%d_a' % bi, (B, ohw[0], ohw[1], c1.cout))
                self._conv_fwd(c1, x, xhw, ya, True, sign=sa, pair=x3)
                sk = x
                if ds is not None:
                    sk = self._act('b%d_ds' % bi, (B, ohw[0], ohw[1], ds.cout))
                    self._conv_fwd(ds, x, xhw, sk, False, pair=x3)
                self._conv_fwd(c2, ya, ohw, y, True, res=sk, sign=so, pair=x3)
            acts['b%d' % bi] = (tuple(x.shape), xhw, ohw, xs, sa)
            x, xhw, xs = y, ohw, so
        acts['last'], acts['last_sign'] = (x, xhw), xs
        return self._head_fwd(x, xhw, B), acts

    def _backward(self, acts, dl, std):
        """d(loss)/d(x01) fp32 NCHW from the fp32 loss gradient dl [B][classes] and the `acts` of a keep=True forward."""
        B = acts['in_shape'][0]
        x3 = self.x3
        dz = self._head_bwd(acts, dl, B)             # masked gradient at the last block's output
        for bi in range(len(self.basic) - 1, -1, -1):
            c1, c2, ds = self.basic[bi]
            xshape, xhw, ohw, mx, ma = acts['b%d' % bi]
            dx = self._get('g_x%d' % bi, xshape)
            if self._basic_ok(c1, c2, ds, xhw, B):
                self._basic(dz, c2.w_bwd_frag, c1.w_bwd_frag, None, None, ma, mx, dx, B, xhw, c1.cin, c2.bwd[0][1], True)
            else:
                dza = self._act('g_a_%dx%d' % (ohw[0], c1.cout), (B, ohw[0], ohw[1], c1.cout))
                self._conv_bwd(c2, dz, ohw, dza, ohw, mask=ma, pair=x3)
                if ds is None:
                    self._conv_bwd(c1, dza, ohw, dx, xhw, res=dz, mask=mx, pair=x3)          # identity skip
                else:
                    self._conv_bwd(c1, dza, ohw, dx, xhw, mask=mx, pair=x3)
                    self._conv_bwd(ds, dz, ohw, dx, xhw, res=dx, mask=mx, pair=x3)           # accumulate the projection skip
            dz = dx
        return self._stem_bwd(acts, dz, std)


# the widths the kernel serves, and those whose identity blocks take the fused launch by default (see `basic_block_widths`).  Measured
# at B = 256 (profiles/basic_block_ab.json; us, median (min-max), fused against the two launches): 64 @ 56 x 56 forward 200.3
# (198.6-211.4) against 256.4 (254.7-259.5), backward 184.1 (182.7-186.7) against 260.2 (258.5-261.0); 128 @ 28 x 28 forward 158.7
# (157.0-163.2) against 172.8 (169.2-176.6), backward 153.0 (152.0-153.8) against 172.5 (172.1-172.9): both widths meet the rule
BASIC_BLOCK_SERVED = (64, 128)
BASIC_BLOCK_WIDTHS = (64, 128)
