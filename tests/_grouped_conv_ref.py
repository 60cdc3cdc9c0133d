"""What the grouped-convolution tests share (tests/test_grouped_conv_tables_cpu.py, tests/test_grouped_conv_gpu.py): the cases, the
operands, the fp64 references -- the right one and the two wrong ones that prove a test sees the group structure -- and the launch
semantics of rart_conv3x3_grouped_* restated on the host over `_Conv`'s slice tables."""
import numpy as np
import torch
import torch.nn.functional as F

CASES = [(64, 4), (64, 8), (64, 16), (64, 32), (128, 64)]          # (channels, group width): every case has at least two slices
B = 3
BF16_REL, BF16_ABS = 2.0 ** -8, 1e-6        # tests/test_engine_gpu.py::test_conv_kernel_forward_and_backward_layerwise
PAIR_REL = 2.5e-5                           # tests/test_engine_x3_gpu.py::test_pair_gemm_kernel_vs_fp64 (of max |ref|)


def make_layer(C, gw, stride, seed=0):
    """conv (grouped 3x3, pad 1) + eval BatchNorm with non-trivial statistics.  The BatchNorm bias is pushed up so that about nine
    outputs in ten are positive: the ReLU still clamps thousands of outputs, and a wrong reference cannot agree with the right one by
    both being clamped to zero (the 90 % proof below counts every output)."""
    g = torch.Generator().manual_seed(1000 * C + 10 * gw + stride + seed)
    conv = torch.nn.Conv2d(C, C, 3, stride=stride, padding=1, groups=C // gw, bias=False)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * gw)) ** 0.5)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(C, generator=g) * 0.5 + 0.75)
        bn.weight.copy_(torch.rand(C, generator=g) * 0.5 + 0.75)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.1 + 2.0)
    return conv, bn.eval()


def stored(t, split):
    """fp32 -> the value the storage holds, as fp64: bf16(t), or the pair hi + lo"""
    hi = t.to(torch.bfloat16)
    if not split:
        return hi.double()
    return hi.double() + (t - hi.float()).to(torch.bfloat16).double()


def inputs(C, hw, seed, density=0.95):
    """-> (x fp32 NCHW, mask bool NCHW with `density` ones)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, hw[0], hw[1], generator=g)
    return x, torch.rand(B, C, hw[0], hw[1], generator=g) < density


def shifted(w, gw):
    """every group's filters moved to the next group"""
    return torch.roll(w, gw, 0)


def dense_weight(w, groups):
    """the filters of a convolution that ignores `groups`: every output channel applies its gw filter planes to EVERY group of the input"""
    return w.repeat(1, groups, 1, 1)


def ref_forward(x, w, b, stride, groups, relu=True):
    """fp64; groups = 1 with w = `dense_weight`: the dense wrong reference"""
    y = F.conv2d(x, w, None, stride, 1, 1, groups) + b.view(1, -1, 1, 1)
    return y.clamp_min(0) if relu else y


def ref_backward(dz, w, in_hw, stride, groups, mask=None):
    dx = torch.nn.grad.conv2d_input((dz.shape[0], w.shape[1] * groups, in_hw[0], in_hw[1]), w, dz, stride, 1, 1, groups)
    return dx if mask is None else dx * mask


def bf16_violations(got, ref):
    return (got - ref).abs() > ref.abs() * BF16_REL + BF16_ABS


def pair_violations(got, ref):
    return (got - ref).abs() > PAIR_REL * ref.abs().max()


def table_planes(rows, k, split):
    """`_Conv`'s row tables [slices][64][K] (or [hi | lo | hi] columns) -> fp64 [slices][64][K], the value hi (+ lo)"""
    t = rows.double()
    return t[:, :, :k] + t[:, :, k:2 * k] if split else t


def apply_tables(tab, S, taps, src, grid, stride=1, dst_hw=None, dst_stride=1, dst_org=(0, 0), fill=0.0):
    """The launch of rart_conv3x3_grouped_* on the host in fp64: tab [slices][>= S][len(taps) * S], src NCHW; grid pixel (y, x) reads src
    at (y * stride + dy, x * stride + dx) per tap (zero outside) and writes dst at (y * dst_stride + oy, x * dst_stride + ox); the rest of
    dst keeps `fill`."""
    n, C, h, w = src.shape
    dst_hw = dst_hw or grid
    out = torch.full((n, C, dst_hw[0], dst_hw[1]), fill, dtype=torch.float64)
    xp = F.pad(src, (1, 1, 1, 1))
    gy, gx = torch.arange(grid[0]) * stride, torch.arange(grid[1]) * stride
    for i in range(C // S):
        acc = torch.zeros(n, S, grid[0], grid[1], dtype=torch.float64)
        for t, (dy, dx) in enumerate(taps):
            patch = xp[:, i * S:(i + 1) * S][:, :, (gy + dy + 1)][:, :, :, (gx + dx + 1)]
            acc += torch.einsum('oc,ncyx->noyx', tab[i, :S, t * S:(t + 1) * S], patch)
        out[:, i * S:(i + 1) * S, dst_org[0]::dst_stride, dst_org[1]::dst_stride][:, :, :grid[0], :grid[1]] = acc
    return out


def frag_decode(frag, ns, S, k):
    """the fragment-ordered table of rart_conv3x3_grouped_* -> [slices][S][K] (include/robustart_hip.h)"""
    return frag.reshape(ns, k // 16, S // 32, 2, 32, 8).permute(0, 2, 4, 1, 3, 5).reshape(ns, S, k)


def pack_bits(mask_nchw):
    """bool NCHW -> the 1-bit NHWC tensor (bit e & 7 of byte e >> 3 for element offset e)"""
    return torch.from_numpy(np.packbits(mask_nchw.permute(0, 2, 3, 1).contiguous().numpy().reshape(-1), bitorder='little'))


def unpack_bits(bits, shape_nhwc):
    return torch.from_numpy(np.unpackbits(bits.numpy(), bitorder='little')).bool().reshape(shape_nhwc).permute(0, 3, 1, 2)
