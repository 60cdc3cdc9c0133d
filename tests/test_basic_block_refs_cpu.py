"""The fp64 references of the fused BasicBlock kernel (csrc/basic_block.hip), which tests/test_basic_block_gpu.py imports, checked here
against F.conv2d / torch.nn.grad.conv2d_input -- and the proof that the GPU test's bound separates a right kernel from the wrong ones
this kernel can be: an fp32 emulation of the fused arithmetic stays inside it, while an intermediate computed on the halo ring
(instead of zero padding), a dropped residual and a backward with unflipped taps all miss it at a large share of the outputs.

    forward :  out = relu(W2 * bf16(relu(W1 * x + b1)) + b2 + x)
    backward:  dx  = m_in . (W1^T * bf16(m_mid . (W2^T * g)) + g)
    bound   :  |err| <= |ref| 2^-8 + 2 * 2^-8 * max|intermediate| * max|second conv's weights| + 1e-6
"""
import pytest
import torch
import torch.nn.functional as F

CASES = [(64, 7, 7), (64, 9, 20), (128, 6, 14), (64, 17, 56)]        # (C, h, w)
N = 2


def bf16r(t):
    """round to bf16 (nearest even), keep the dtype"""
    return t.float().bfloat16().to(t.dtype)


def make_inputs(c, n, h, w, seed):
    """-> dict of NCHW fp64 tensors that are exact in bf16 (x, w1, w2, g) or fp32 (b1, b2): x = relu(N(0,1)); He-scaled weights; b1
    uniform in [0.25, 0.75] (a wrongly padded intermediate is visibly positive); b2 = 0.1 N(0,1); g = N(0,1) under a random mask."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)         # noqa: E731
    std = (2.0 / (9 * c)) ** 0.5
    return dict(x=bf16r(rn(n, c, h, w).clamp_min(0)), w1=bf16r(rn(c, c, 3, 3) * std), w2=bf16r(rn(c, c, 3, 3) * std),
                b1=(torch.rand(c, generator=gen, dtype=torch.float64) * 0.5 + 0.25).float().double(), b2=(0.1 * rn(c)).float().double(),
                g=bf16r(rn(n, c, h, w) * (torch.rand(n, c, h, w, generator=gen) < 0.6)))


def ref_forward(x, w1, w2, b1, b2):
    """fp64 -> (pre-activation a of the intermediate, the stored intermediate bf16(relu(a)), out before its final rounding)"""
    a = F.conv2d(x, w1, b1, padding=1)
    mid = bf16r(a.clamp_min(0))
    return a, mid, (F.conv2d(mid, w2, b2, padding=1) + x).clamp_min(0)


def ref_backward(g, w1, w2, m_mid, m_in):
    """fp64 -> (the stored intermediate gradient bf16(m_mid . W2^T g), dx before its final rounding); m_in may be None"""
    t = bf16r(conv_t(g, w2) * m_mid)
    dx = conv_t(t, w1) + g
    return t, dx if m_in is None else dx * m_in


def conv_t(g, w):
    """backward-to-input of the stride-1 pad-1 3x3 convolution with weight w [out][in][3][3]: a convolution with the taps FLIPPED and the
    channel roles swapped"""
    return F.conv2d(g, w.flip(2, 3).transpose(0, 1), padding=1)


def bound(ref, mid, w_second):
    """the bound of the GPU test, elementwise: one bf16 rounding of the stored result + two flipped roundings of the intermediate"""
    return ref.abs() * 2.0 ** -8 + 2 * 2.0 ** -8 * mid.abs().max().item() * w_second.abs().max().item() + 1e-6


def border(t):
    """the outermost rows and columns of NCHW t, as a boolean mask"""
    m = torch.zeros_like(t, dtype=torch.bool)
    m[:, :, 0], m[:, :, -1], m[:, :, :, 0], m[:, :, :, -1] = True, True, True, True
    return m


@pytest.fixture(scope='module', params=CASES, ids=lambda c: '%dx%dx%d' % c)
def case(request):
    c, h, w = request.param
    d = make_inputs(c, N, h, w, seed=c + 7 * h + w)
    d['a'], d['mid'], d['out'] = ref_forward(d['x'], d['w1'], d['w2'], d['b1'], d['b2'])
    d['m_mid'], d['m_in'] = (d['mid'] > 0).double(), (d['x'] > 0).double()
    d['t'], d['dx'] = ref_backward(d['g'], d['w1'], d['w2'], d['m_mid'], d['m_in'])
    return d


def test_references_against_autograd(case):
    """the references' convolutions are torch's; their backward is autograd's of the forward with the rounding taken out"""
    d = case
    x = d['x'].clone().requires_grad_(True)
    a = F.conv2d(x, d['w1'], d['b1'], padding=1).clamp_min(0)
    out = (F.conv2d(a, d['w2'], d['b2'], padding=1) + x)
    gx, = torch.autograd.grad(out, x, d['g'])
    t = conv_t(d['g'], d['w2']) * (a > 0)
    assert torch.allclose(t, torch.nn.grad.conv2d_input(d['x'].shape, d['w2'], d['g'], padding=1) * (a > 0), rtol=0, atol=1e-12)
    assert torch.allclose(conv_t(t, d['w1']) + d['g'], gx, rtol=0, atol=1e-12 * gx.abs().max().item())


def test_fp32_emulation_of_the_fused_arithmetic_stays_inside_the_bound(case):
    d = case
    f = {k: v.float() for k, v in d.items()}
    mid = bf16r(F.conv2d(f['x'], f['w1'], f['b1'], padding=1).clamp_min(0))
    out = bf16r((F.conv2d(mid, f['w2'], f['b2'], padding=1) + f['x']).clamp_min(0)).double()
    r_f = ((out - d['out']).abs() / bound(d['out'], d['mid'], d['w2'])).max().item()
    t = bf16r(conv_t(f['g'], f['w2']) * f['m_mid'])
    dx = bf16r((conv_t(t, f['w1']) + f['g']) * f['m_in']).double()
    r_b = ((dx - d['dx']).abs() / bound(d['dx'], d['t'], d['w1'])).max().item()
    print('fp32 emulation, worst error / bound: forward %.3f backward %.3f' % (r_f, r_b))
    assert r_f <= 1.0 and r_b <= 1.0


def test_intermediate_on_the_halo_ring_misses_the_bound_at_the_border(case):
    """the wrong kernel: relu(W1 * padded x + b1) on the ring around the image instead of the second convolution's zero padding"""
    d = case
    ring = bf16r(F.conv2d(F.pad(d['x'], (2, 2, 2, 2)), d['w1'], d['b1']).clamp_min(0))           # (h + 2) x (w + 2)
    out = (F.conv2d(ring, d['w2'], d['b2']) + d['x']).clamp_min(0)
    miss = (out - d['out']).abs() > bound(d['out'], d['mid'], d['w2'])
    b = border(out)
    share = miss[b].double().mean().item()
    print('halo-ring variant: %.1f %% of the border outputs past the bound (interior: %d)' % (100 * share, int(miss[~b].sum())))
    assert share >= 0.5 and not miss[~b].any()


def test_dropped_residual_misses_the_bound(case):
    d = case
    out = F.conv2d(d['mid'], d['w2'], d['b2'], padding=1).clamp_min(0)
    share = ((out - d['out']).abs() > bound(d['out'], d['mid'], d['w2'])).double().mean().item()
    print('dropped-residual variant: %.1f %% of all outputs past the bound' % (100 * share))
    assert share >= 0.25


def test_backward_with_unflipped_taps_misses_the_bound(case):
    """the wrong backward: the transposed tables with the FORWARD's taps.  Measured at the four cases: 49 - 50 % of the border outputs,
    which is every output m_in leaves alive (it zeroes about half of them, right or wrong), so the threshold of 25 % stands."""
    d = case
    unflipped = lambda g, w: F.conv2d(g, w.transpose(0, 1), padding=1)                            # noqa: E731
    t = bf16r(unflipped(d['g'], d['w2']) * d['m_mid'])
    dx = (unflipped(t, d['w1']) + d['g']) * d['m_in']
    miss = (dx - d['dx']).abs() > bound(d['dx'], d['t'], d['w1'])
    share = miss[border(dx)].double().mean().item()
    print('unflipped-taps backward: %.1f %% of the border outputs past the bound' % (100 * share))
    assert share >= 0.25


def test_few_intermediates_sit_at_the_sign_threshold(case):
    """the GPU test compares the intermediate's sign bits with the fp64 sign where |a| >= 1e-4 max|a|: that excludes next to nothing"""
    a = case['a']
    share = (a.abs() < 1e-4 * a.abs().max()).double().mean().item()
    print('intermediates with |a| < 1e-4 max|a|: %.2e' % share)
    assert share < 1e-3
