"""fp64 references for the streaming attention tests: soft-max attention and its autograd on the values a pair represents, the spike
inputs that move the running maximum, and the yardsticks of the existing attention tests."""
import functools

import torch

B, H, HD = 2, 3, 64
D = H * HD


def split(t):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


def f64(p):
    return p[0].double() + p[1].double()


def attention64(qkv, n, T, heads=H):
    """qkv fp64 [n*T][3*heads*64] -> out fp64 [n*T][heads*64]"""
    q = qkv.view(n, T, 3, heads, HD).permute(2, 0, 3, 1, 4)
    return (torch.softmax(q[0] @ q[1].transpose(-1, -2) / 8.0, -1) @ q[2]).permute(0, 2, 1, 3).reshape(n * T, heads * HD)


# (spiked key, first query of the band of 40 queries it dominates) at T = 577: key 0, one in the middle chunk, T - 1, and one in
# the last partial 32-key tile -- at 577 tokens that tile holds key 576 = T - 1 alone, so the fourth case spikes it for the band
# that ends in the last, partial QUERY tile
SPIKE_T = 577
SPIKES = {'first': (0, 100), 'middle': (300, 500), 'last': (576, 30), 'partial': (576, 537)}
BAND = 40


SCALE = {'pair': 1.5, 'bf16': 0.7}          # the input scales of the resident kernels' tests (test_vit_x3_gpu.py, test_vit_gpu.py)
# The spike cases multiply one K row by 8, and the error of a pair contraction (three products: the lo . lo term is dropped) grows with
# |q| |k|.  At the pair tests' scale 1.5 the spiked scores reach 200 and the dropped term ALONE, with every other step exact, puts the
# forward 3.0e-5 of scale from fp64 (three_product_forward_error below; the bound is 2.5e-5): no three-product kernel can pass there.
# At 0.7 the same figure is a quarter of that ((0.7 / 1.5)^2), test_att_stream_cpu.py holds it under half the bound, and the spiked
# key still stands 18 above every other score of its band (a factor e^18 between the maxima before and after its tile).
SPIKE_SCALE = 0.7


def make_inputs(T, seed, n=B, spike=None, scale=SCALE['pair']):
    """fp32 CPU tensors (qkv [n*T][3D], dout [n*T][D]); with `spike`, K row `key` of every image and head is a row of the input's
    scale times 8, along the direction the band's queries lean to, so that the key's score stands far above every other score of
    those queries"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n * T, 3 * D, generator=g) * scale
    dout = torch.randn(n * T, D, generator=g)
    if spike is not None:
        key, q0 = SPIKES[spike]
        v = qkv.view(n, T, 3, H, HD)
        band = v[:, q0:q0 + BAND, 0]                                   # [n][BAND][H][HD]
        base = torch.randn(n, 1, H, HD, generator=g)                   # a common direction the band's queries lean to
        band.copy_(0.5 * band + scale * base)
        v[:, key, 1] = 8 * scale * base[:, 0]
    return qkv, dout


@functools.lru_cache(maxsize=None)
def case(T, seed, n=B, spike=None):
    """the shared reference of one case, computed once: pair and bf16 inputs on the CPU with the fp64 forward and autograd of each.
    -> dict(pair=(qkv [2][..], dout [2][..], out64, dqkv64), bf16=(qkv, dout, out64, dqkv64))"""
    res = {}
    for name in ('pair', 'bf16'):
        qkv, dout = make_inputs(T, seed, n, spike, SCALE[name] if spike is None else SPIKE_SCALE)
        if name == 'pair':
            qs, ds = split(qkv), split(dout)
            q64, d64 = f64(qs), f64(ds)
        else:
            qs, ds = qkv.to(torch.bfloat16), dout.to(torch.bfloat16)
            q64, d64 = qs.double(), ds.double()
        q64 = q64.requires_grad_(True)
        o64 = attention64(q64, n, T)
        (o64 * d64).sum().backward()
        res[name] = (qs, ds, o64.detach(), q64.grad)
    return res


def running_max_moves(qkv64, T, key, q0, n=B):
    """for the band's queries: the maximum over 32-key tiles [0, tile of `key`) is below the spiked score, i.e. a kernel that walks the
    keys in order changes its running maximum at the spiked key's tile (for key 0: every later tile stays below it)"""
    q = qkv64.view(n, T, 3, H, HD).permute(2, 0, 3, 1, 4)
    s = (q[0] @ q[1].transpose(-1, -2) / 8.0)[:, :, q0:q0 + BAND]       # [n][H][BAND][T]
    spike = s[..., key]
    others = torch.cat([s[..., :key], s[..., key + 1:]], -1).max(-1).values
    return bool((spike > others + 4).all()), float((spike - others).min())


def three_product_forward_error(qs, o64, T, n=B):
    """the forward error (of scale) that the pair format alone leaves: scores as hi . hi + hi . lo + lo . hi in fp64, everything else exact"""
    h, l = (t.double().view(n, T, 3, H, HD).permute(2, 0, 3, 1, 4) for t in (qs[0], qs[1]))
    s3 = h[0] @ h[1].transpose(-1, -2) + h[0] @ l[1].transpose(-1, -2) + l[0] @ h[1].transpose(-1, -2)
    o = (torch.softmax(s3 / 8.0, -1) @ (h[2] + l[2])).permute(0, 2, 1, 3).reshape(n * T, D)
    return rel_max(o, o64)


def rel_max(got, want, whole=None):
    """max error over the scale of `want`.  A part that is exactly zero (T = 1: the soft-max of one key is constant, dQ = dK = 0) has no
    scale of its own: it is measured on the scale of the `whole` gradient it is stored in, which is what the next GEMM sees"""
    scale = want.abs().max().item()
    if scale == 0 and whole is not None:
        scale = whole.abs().max().item()
    return (got - want).abs().max().item() / scale


def cos_rel(got, want, whole=None):
    """(cosine, relative L2 error); for an exactly zero part the cosine is 1 by convention and the error is relative to `whole`"""
    a, b = got.flatten().double(), want.flatten().double()
    if b.norm().item() == 0 and whole is not None:
        return 1.0, (a.norm() / whole.flatten().double().norm()).item()
    return (a @ b / (a.norm() * b.norm())).item(), ((a - b).norm() / b.norm()).item()
