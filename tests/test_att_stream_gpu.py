"""The four streaming attention entries (csrc/vit_stream.hip) on the GPU against fp64 soft-max attention and its autograd on the
values the operands represent (tests/_att_stream_ref.py), with the bounds the resident kernels are held to:
  pair forward <= 2.5e-5 of scale, pair backward dQ / dK / dV <= 3e-5 of scale each          (test_vit_x3_gpu.py)
  bf16 forward < 0.02 * scale + 2e-2, bf16 backward cos > 0.9995 and rel < 0.03 per part     (test_vit_gpu.py)
Token counts on both sides of the resident limit, of the 64-row chunk and of the eight-tile block; spiked keys that move the
running maximum; poisoned rows around the operands and guarded rows around the results; bit-level batch independence."""
import pytest
import torch

import _att_stream_ref as R

pytestmark = pytest.mark.gpu
B, H, HD, D = R.B, R.H, R.HD, R.D
SENTINEL = 3.0
EXTRA = 40                # rows behind B*T of every pair plane and every result


def _lib_():
    from robustart_amd import _lib
    return _lib, _lib.load()


def _padded(t, rows, fill):
    """t [.., r, c] with `rows` more rows of `fill` behind it, on the GPU"""
    pad = torch.full(t.shape[:-2] + (rows, t.shape[-1]), fill, dtype=t.dtype)
    return torch.cat([t, pad], -2).contiguous().cuda()


def _result(pair, rows, cols):
    """NaN where the kernel has to write, the sentinel behind the last token"""
    out = torch.full(((2,) if pair else ()) + (rows + EXTRA, cols), float('nan'), dtype=torch.bfloat16, device='cuda')
    out[..., rows:, :] = SENTINEL
    return out


def _value(pair, t, rows):
    return (R.f64(t) if pair else t.double())[:rows].cpu()


def run(storage, c, n, T):
    """forward and backward of one case through the stream entries -> (out fp64, dqkv fp64), after the guards around them"""
    _lib, lib = _lib_()
    pair = storage == 'pair'
    qs, ds, o64, g64 = c[storage]
    rows, sp = n * T, _lib.stream_ptr()
    # operands: NaN rows behind the pair planes, 256 slack rows of 7.0 behind the bf16 qkv
    qkv = _padded(qs, EXTRA, float('nan')) if pair else _padded(qs, 256, 7.0)
    dout = _padded(ds, EXTRA, float('nan'))
    att_in = R.split(o64.float()) if pair else o64.to(torch.bfloat16)              # O as the engine hands it: the forward's output, rounded
    att_in = _padded(att_in, EXTRA, float('nan'))
    out, dqkv = _result(pair, rows, D), _result(pair, rows, 3 * D)
    stats = torch.full((n * H * ((T + 31) // 32 * 32) * 4 + 64,), float('nan'), dtype=torch.float32, device='cuda')
    hl = (lambda t: (_lib.ptr(t[0]), _lib.ptr(t[1]))) if pair else (lambda t: (_lib.ptr(t),))
    fwd = lib.rart_vit_attention_stream_pair if pair else lib.rart_vit_attention_stream
    bwd = lib.rart_vit_attention_bwd_stream_pair if pair else lib.rart_vit_attention_bwd_stream
    _lib.check(fwd(*hl(qkv), *hl(out), n, T, H, HD, sp))
    _lib.check(bwd(*hl(qkv), *hl(att_in), *hl(dout), *hl(dqkv), _lib.ptr(stats), n, T, H, HD, sp))
    torch.cuda.synchronize()
    for name, t in (('out', out), ('dqkv', dqkv)):
        assert torch.isfinite(t[..., :rows, :].float()).all(), '%s: a row in range was not written, or not finite' % name
        assert (t[..., rows:, :] == SENTINEL).all(), '%s: written past the last token' % name
    st = stats[:n * H * ((T + 31) // 32 * 32) * 4]
    assert torch.isfinite(st).all() and torch.isnan(stats[st.numel():]).all()
    return _value(pair, out, rows), _value(pair, dqkv, rows), out, dqkv


def torch_fp32(storage, c, n, T):
    """torch's fp32 attention and autograd on the same values, for the printed comparison"""
    qs, ds, _, _ = c[storage]
    q = (R.f64(qs) if storage == 'pair' else qs.double()).float().cuda().requires_grad_(True)
    d = (R.f64(ds) if storage == 'pair' else ds.double()).float().cuda()
    v = q.view(n, T, 3, H, HD).permute(2, 0, 3, 1, 4)
    o = (torch.softmax(v[0] @ v[1].transpose(-1, -2) / 8.0, -1) @ v[2]).permute(0, 2, 1, 3).reshape(n * T, D)
    (o * d).sum().backward()
    return o.detach().double().cpu(), q.grad.double().cpu()


def check(storage, c, n, T, tag):
    got_o, got_g, _, _ = run(storage, c, n, T)
    t_o, t_g = torch_fp32(storage, c, n, T)
    _, _, o64, g64 = c[storage]
    if storage == 'pair':
        e, et = R.rel_max(got_o, o64), R.rel_max(t_o, o64)
        print('stream pair %s T=%d forward: max err %.2e of scale (torch fp32: %.2e)' % (tag, T, e, et))
        fails = [] if e <= 2.5e-5 else [('forward', e)]
        for name, lo in (('dQ', 0), ('dK', D), ('dV', 2 * D)):
            e, et = R.rel_max(got_g[:, lo:lo + D], g64[:, lo:lo + D], g64), R.rel_max(t_g[:, lo:lo + D], g64[:, lo:lo + D], g64)
            print('stream pair %s T=%d backward %s: max err %.2e of scale (torch fp32: %.2e)' % (tag, T, name, e, et))
            if not e <= 3e-5:
                fails.append((name, e))
        assert not fails, fails
    else:
        scale = o64.abs().max().item()
        e, et = (got_o - o64).abs().max().item(), (t_o - o64).abs().max().item()
        print('stream bf16 %s T=%d forward: max err %.3g at scale %.3f (torch fp32: %.2e)' % (tag, T, e, scale, et))
        fails = [] if e < 0.02 * scale + 2e-2 else [('forward', e)]
        for name, lo in (('dQ', 0), ('dK', D), ('dV', 2 * D)):
            cos, rel = R.cos_rel(got_g[:, lo:lo + D], g64[:, lo:lo + D], g64)
            cos_t, rel_t = R.cos_rel(t_g[:, lo:lo + D], g64[:, lo:lo + D], g64)
            print('stream bf16 %s T=%d backward %s: 1 - cos %.2e, rel %.2e (torch fp32: %.2e, %.2e)' % (tag, T, name, 1 - cos, rel, 1 - cos_t, rel_t))
            if not (cos > 0.9995 and rel < 0.03):
                fails.append((name, cos, rel))
        assert not fails, fails


# above the resident limit: 225 (one more token), 256 / 257 (a full chunk and one more: 8 tiles in one block, 9 in two), 449 (15 tiles,
# an odd count over two blocks, a partial chunk), 577 (ViT-B/16 at 384: 19 tiles over three blocks); below it, through the same
# entries: 1, 33 (a partial second tile in one chunk), 197, 224
@pytest.mark.parametrize('T', [225, 256, 257, 449, 577, 1, 33, 197, 224])
@pytest.mark.parametrize('storage', ['pair', 'bf16'])
def test_stream_attention_forward_and_backward_vs_fp64(storage, T):
    check(storage, R.case(T, 1000 + T), B, T, 'random')


@pytest.mark.parametrize('spike', sorted(R.SPIKES))
@pytest.mark.parametrize('storage', ['pair', 'bf16'])
def test_stream_attention_rescale_branch_on_spiked_keys(storage, spike):
    """one K row 8 x the input scale along the direction a band of queries leans to: the band's running maximum moves at the spiked
    key's tile (tests/test_att_stream_cpu.py checks that on the inputs), so O and the running sum are rescaled by a factor far from 1"""
    check(storage, R.case(R.SPIKE_T, 900, spike=spike), B, R.SPIKE_T, 'spike ' + spike)


def test_stream_attention_takes_1025_tokens():
    """beyond every LDS-resident layout: 33 tiles over five blocks, 17 chunks"""
    for storage in ('pair', 'bf16'):
        check(storage, R.case(1025, 77, n=1), 1, 1025, 'long')


@pytest.mark.parametrize('T', [257, 577])
@pytest.mark.parametrize('storage', ['pair', 'bf16'])
def test_stream_attention_is_batch_independent_and_reproducible(storage, T):
    """image 1 alone == row block 1 of the three-image launch, bit for bit, forward and backward; two launches of one input agree
    bit for bit"""
    c3 = R.case(T, 4000 + T, n=3)
    qs, ds, o64, g64 = c3[storage]
    sl = slice(T, 2 * T)
    c1 = {storage: (qs[..., sl, :].contiguous(), ds[..., sl, :].contiguous(), o64[sl], g64[sl])}
    _, _, out3, dq3 = run(storage, c3, 3, T)
    _, _, out3b, dq3b = run(storage, c3, 3, T)
    _, _, out1, dq1 = run(storage, c1, 1, T)
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(out3), bits(out3b)) and torch.equal(bits(dq3), bits(dq3b))
    assert torch.equal(bits(out1[..., :T, :]), bits(out3[..., sl, :]))
    assert torch.equal(bits(dq1[..., :T, :]), bits(dq3[..., sl, :]))
