"""The entries of csrc/densenet.hip against fp64, one by one, in both storages: the pre-activation (affine + ReLU over a channel prefix
of a wider buffer, dense operand + sign bits out), its backward (write or add into a channel prefix, channels past it untouched), the
pair with the transition's 2x2 average pool folded in, and the slice copy.

Bounds (u = one ulp of the storage relative to the value: 2^-8 for bf16, 2^-16 for the hi + lo pair; 2^-22 covers the fp32 arithmetic,
a fused multiply-add and at most three additions, each within 2^-24 of the magnitudes that enter it):
    forward   |err| <= u |v| + 2^-22 (|s x| + |t|)            (pooled: the mean of that term over the window)
    backward  |err| <= u |v| + 2^-22 (|s d| + |g_old|)
Sign bits are compared exactly: with the stored value (plain form), with the sign of the exact s x + t (pooled form: a fused
multiply-add rounds once, so it keeps that sign).  Every measured maximum is printed beside its bound."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64          # elements (bf16) / bytes (sign tensors) on either side of every written tensor


def _lib():
    from robustart_amd import _lib as L
    return L, L.load()


def _values(shape, pair, g, scale=1.0):
    """-> (fp64 values exactly representable in the storage, hi bf16, lo bf16 or None), on the host"""
    v = torch.randn(shape, generator=g) * scale
    hi = v.to(torch.bfloat16)
    if not pair:
        return hi.double(), hi, None
    lo = (v - hi.float()).to(torch.bfloat16)
    return hi.double() + lo.double(), hi, lo


def _guarded(t, fill):
    """device copy of the host tensor t inside a flat buffer with guard bands -> (buffer, view)"""
    buf = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype).cuda()
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


def _strided(vals_hi, ld, g):
    """rows of C values inside rows of ld elements (the rest random) -> host tensor [rows][ld]"""
    rows, c = vals_hi.shape
    full = torch.randn(rows, ld, generator=g).to(torch.bfloat16)
    full[:, :c] = vals_hi
    return full


def _unpack(sign, rows, c):
    return torch.from_numpy(np.unpackbits(sign.cpu().numpy().reshape(rows, c // 8), axis=-1, bitorder='little')).bool()


def _affine(c, g):
    """(s, t) fp32: signs mixed so that about half of s x + t is negative; channel 0 has s = t = 0, channel 1 gives exact zeros at x = 1"""
    s = (torch.rand(c, generator=g) * 1.0 + 0.5) * (torch.randint(0, 2, (c,), generator=g) * 2 - 1).float()
    t = torch.randn(c, generator=g) * 0.3
    s[0], t[0] = 0.0, 0.0
    s[1], t[1] = 0.75, -0.75
    return s, t


def _ptr(L, t):
    return None if t is None else L.c_void_p(t.data_ptr())


def _call(L, lib, stem, pair, *args):
    """rart_dn_<stem>_{bf16,pair}; an activation is a tuple (hi, lo)"""
    a = []
    for v in args:
        if isinstance(v, tuple):
            a += [_ptr(L, v[0]), _ptr(L, v[1])] if pair else [_ptr(L, v[0])]
        else:
            a.append(_ptr(L, v) if (v is None or torch.is_tensor(v)) else v)
    L.check(getattr(lib, 'rart_dn_%s_%s' % (stem, 'pair' if pair else 'bf16'))(*a, L.stream_ptr()))
    torch.cuda.synchronize()


def _err_vs_bound(got, want, bound):
    """-> max of |got - want| / bound over the finite entries; NaN and Inf positions must agree exactly"""
    fin = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
    assert torch.equal(got[torch.isinf(want)], want[torch.isinf(want)])
    if not fin.any():
        return 0.0
    return ((got[fin] - want[fin]).abs() / bound[fin].clamp_min(1e-300)).max().item()


ROWS = (1, 63, 197, 3 * 49)
U = {False: 2.0 ** -8, True: 2.0 ** -16}


@pytest.mark.parametrize('pair', [False, True])
@pytest.mark.parametrize('c', [32, 96, 224, 1920])
def test_preact_forward_vs_fp64(c, pair):
    L, lib = _lib()
    worst = 0.0
    for rows in ROWS:
        for ld in (c, c + 32, 2 * c):
            g = torch.Generator().manual_seed(rows * 7 + ld)
            xv, xh, xl = _values((rows, c), pair, g)
            s, t = _affine(c, g)
            r0 = rows // 2
            xh[:, 1][::2] = 1.0                                           # exact zeros of s x + t
            xh[r0, 2::3], xh[r0, 3::3] = float('inf'), float('nan')     # one row with +Inf / NaN
            if pair:
                xl[:, 1][::2] = 0.0
                xl[r0, 2::3], xl[r0, 3::3] = 0.0, 0.0
            xv = xh.double() + (xl.double() if pair else 0.0)
            x_hi = _strided(xh, ld, g).cuda()
            x_lo = _strided(xl, ld, g).cuda() if pair else None
            sd, td = s.cuda(), t.cuda()
            yb = [_guarded(torch.zeros(rows, c, dtype=torch.bfloat16), 7.0) for _ in range(2 if pair else 1)]
            sb, sign = _guarded(torch.zeros(rows * c // 8, dtype=torch.uint8), 0xA5)
            _call(L, lib, 'preact', pair, (x_hi, x_lo), ld, sd, td, (yb[0][1], yb[1][1] if pair else None), sign, rows, c)
            stored_hi = yb[0][1].cpu()
            got = stored_hi.double() + (yb[1][1].cpu().double() if pair else 0.0)
            a = s.double() * xv + t.double()
            want = torch.where(a <= 0, torch.zeros_like(a), a)           # a NaN stays a NaN
            bound = U[pair] * want.abs() + 2.0 ** -22 * ((s.double() * xv).abs() + t.double().abs())
            worst = max(worst, _err_vs_bound(got, want, bound))
            assert torch.equal(_unpack(sign, rows, c), stored_hi.float() > 0), (rows, c, ld)
            assert (want[torch.isfinite(want)] == 0).float().mean().item() > 0.3 and (got[:, 1][::2] == 0).all()
            assert all(_guards_intact(b, 7.0) for b, _ in yb) and _guards_intact(sb, 0xA5), (rows, c, ld)
            # without a sign tensor: the same operand
            y2 = [torch.zeros(rows, c, dtype=torch.bfloat16).cuda() for _ in range(2 if pair else 1)]
            _call(L, lib, 'preact', pair, (x_hi, x_lo), ld, sd, td, (y2[0], y2[1] if pair else None), None, rows, c)
            assert all(torch.equal(p.view(torch.int16), q[1].view(torch.int16)) for p, q in zip(y2, yb))
    print('preact %s C = %d: max |err| / bound %.3f (bound 1)' % ('pair' if pair else 'bf16', c, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('pair', [False, True])
@pytest.mark.parametrize('c', [32, 96, 224, 1920])
def test_preact_backward_vs_fp64(c, pair):
    L, lib = _lib()
    worst = 0.0
    for rows in ROWS:
        for ld in (c, c + 32, 2 * c):
            for accumulate in (0, 1):
                for with_s in (True, False):
                    g = torch.Generator().manual_seed(rows * 11 + ld + accumulate)
                    dv, dh, dl = _values((rows, c), pair, g)
                    gv, gh, gl = _values((rows, ld), pair, g)
                    s = (torch.rand(c, generator=g) + 0.5) * (torch.randint(0, 2, (c,), generator=g) * 2 - 1).float()
                    bits = torch.randint(0, 256, (rows * c // 8,), generator=g, dtype=torch.int32).to(torch.uint8)
                    gb = [_guarded(p, 3.0) for p in ((gh, gl) if pair else (gh,))]
                    _call(L, lib, 'preact_bwd', pair, (dh.cuda(), dl.cuda() if pair else None), bits.cuda(), s.cuda() if with_s else None,
                          (gb[0][1], gb[1][1] if pair else None), ld, accumulate, rows, c)
                    out = gb[0][1].cpu().double() + (gb[1][1].cpu().double() if pair else 0.0)
                    sv = s.double() if with_s else torch.ones(c, dtype=torch.float64)
                    contrib = _unpack(bits, rows, c).double() * sv * dv
                    old = gv[:, :c] * accumulate
                    want = contrib + old
                    bound = U[pair] * want.abs() + 2.0 ** -22 * (contrib.abs() + old.abs())
                    worst = max(worst, _err_vs_bound(out[:, :c], want, bound))
                    # the channels >= C of every row and the guard bands: bit-identical to before
                    for (buf, view), before in zip(gb, (gh, gl)):
                        assert torch.equal(view[:, c:].cpu().view(torch.int16), before[:, c:].view(torch.int16)), (rows, c, ld, accumulate)
                        assert _guards_intact(buf, 3.0)
    print('preact_bwd %s C = %d: max |err| / bound %.3f (bound 1)' % ('pair' if pair else 'bf16', c, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('pair', [False, True])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('hw', [(2, 2), (6, 10), (14, 14)])
def test_pool_pair_vs_fp64(hw, n, pair):
    L, lib = _lib()
    h, w = hw
    worst_f = worst_b = 0.0
    for c in (32, 96):
        for ld in (c, c + 32):
            g = torch.Generator().manual_seed(h * 100 + w * 10 + n + ld)
            rows, prow = n * h * w, n * (h // 2) * (w // 2)
            xv, xh, xl = _values((rows, c), pair, g)
            s, t = _affine(c, g)
            x_hi = _strided(xh, ld, g).cuda()
            x_lo = _strided(xl, ld, g).cuda() if pair else None
            yb = [_guarded(torch.zeros(prow, c, dtype=torch.bfloat16), 7.0) for _ in range(2 if pair else 1)]
            sb, sign = _guarded(torch.zeros(rows * c // 8, dtype=torch.uint8), 0xA5)
            _call(L, lib, 'preact_pool2', pair, (x_hi, x_lo), ld, s.cuda(), t.cuda(), (yb[0][1], yb[1][1] if pair else None), sign, n, h, w, c)
            got = yb[0][1].cpu().double() + (yb[1][1].cpu().double() if pair else 0.0)
            a = s.double() * xv + t.double()
            act = a.clamp_min(0).view(n, h // 2, 2, w // 2, 2, c)
            mag = ((s.double() * xv).abs() + t.double().abs()).view(n, h // 2, 2, w // 2, 2, c)
            want = act.mean((2, 4)).reshape(prow, c)
            bound = U[pair] * want.abs() + 2.0 ** -22 * mag.mean((2, 4)).reshape(prow, c)
            worst_f = max(worst_f, _err_vs_bound(got, want, bound))
            assert torch.equal(_unpack(sign, rows, c), a > 0), (hw, n, c, ld)          # full resolution
            assert all(_guards_intact(b, 7.0) for b, _ in yb) and _guards_intact(sb, 0xA5)
            # backward: d / 4 under the bits, write and add
            for accumulate in (0, 1):
                for with_s in (True, False):
                    dv, dh, dl = _values((prow, c), pair, g)
                    gv, gh, gl = _values((rows, ld), pair, g)
                    gb = [_guarded(p, 3.0) for p in ((gh, gl) if pair else (gh,))]
                    _call(L, lib, 'preact_pool2_bwd', pair, (dh.cuda(), dl.cuda() if pair else None), sign, s.cuda() if with_s else None,
                          (gb[0][1], gb[1][1] if pair else None), ld, accumulate, n, h, w, c)
                    out = gb[0][1].cpu().double() + (gb[1][1].cpu().double() if pair else 0.0)
                    up = dv.view(n, h // 2, 1, w // 2, 1, c).expand(n, h // 2, 2, w // 2, 2, c).reshape(rows, c)
                    sv = s.double() if with_s else torch.ones(c, dtype=torch.float64)
                    contrib = (a > 0).double() * sv * up / 4
                    old = gv[:, :c] * accumulate
                    want_g = contrib + old
                    worst_b = max(worst_b, _err_vs_bound(out[:, :c], want_g, U[pair] * want_g.abs() + 2.0 ** -22 * (contrib.abs() + old.abs())))
                    for (buf, view), before in zip(gb, (gh, gl)):
                        assert torch.equal(view[:, c:].cpu().view(torch.int16), before[:, c:].view(torch.int16))
                        assert _guards_intact(buf, 3.0)
    print('pool2 %s %dx%d n = %d: forward max |err| / bound %.3f, backward %.3f (bound 1)' % ('pair' if pair else 'bf16', h, w, n, worst_f, worst_b))
    assert worst_f <= 1.0 and worst_b <= 1.0


@pytest.mark.parametrize('pair', [False, True])
def test_slice_copy_is_a_bit_copy_of_the_slice_alone(pair):
    L, lib = _lib()
    for rows, c, ld_s, ld_d in ((1, 32, 32, 64), (197, 64, 256, 64), (147, 96, 128, 224)):
        g = torch.Generator().manual_seed(rows)
        src = [torch.randn(rows, ld_s, generator=g).to(torch.bfloat16) for _ in range(2 if pair else 1)]
        before = [torch.randn(rows, ld_d, generator=g).to(torch.bfloat16) for _ in range(2 if pair else 1)]
        db = [_guarded(p, 5.0) for p in before]
        _call(L, lib, 'copy', pair, (src[0].cuda(), src[1].cuda() if pair else None), ld_s, (db[0][1], db[1][1] if pair else None), ld_d, rows, c)
        for s_, b_, (buf, view) in zip(src, before, db):
            assert torch.equal(view[:, :c].cpu().view(torch.int16), s_[:, :c].view(torch.int16))
            assert torch.equal(view[:, c:].cpu().view(torch.int16), b_[:, c:].view(torch.int16)) and _guards_intact(buf, 5.0)


def test_offsets_past_2_31_elements():
    """a row stride that puts the last rows beyond 2^31 elements (the concat buffer of a large batch): forward reads, backward adds there"""
    L, lib = _lib()
    rows, c, ld = 70000, 32, 32768                      # 2.29e9 elements; only the prefixes are touched
    g = torch.Generator().manual_seed(3)
    xv, xh, _ = _values((rows, c), False, g)
    s, t = _affine(c, g)
    big = torch.empty(rows * ld, dtype=torch.bfloat16, device='cuda')
    big.view(rows, ld)[:, :c] = xh.cuda()
    y = torch.zeros(rows, c, dtype=torch.bfloat16, device='cuda')
    sign = torch.zeros(rows * c // 8, dtype=torch.uint8, device='cuda')
    _call(L, lib, 'preact', False, (big, None), ld, s.cuda(), t.cuda(), (y, None), sign, rows, c)
    a = s.double() * xv + t.double()
    want = a.clamp_min(0)
    e = _err_vs_bound(y.cpu().double(), want, 2.0 ** -8 * want.abs() + 2.0 ** -22 * ((s.double() * xv).abs() + t.double().abs()))
    assert torch.equal(_unpack(sign, rows, c), y.cpu().float() > 0)
    dv, dh, _ = _values((rows, c), False, g)
    old = big.view(rows, ld)[:, :c].cpu().double()
    tail_before = big.view(rows, ld)[-1, c:c + 64].clone()
    _call(L, lib, 'preact_bwd', False, (dh.cuda(), None), sign, None, (big, None), ld, 1, rows, c)
    contrib = (y.cpu().float() > 0).double() * dv
    want_g = contrib + old
    e2 = _err_vs_bound(big.view(rows, ld)[:, :c].cpu().double(), want_g, 2.0 ** -8 * want_g.abs() + 2.0 ** -22 * (contrib.abs() + old.abs()))
    print('rows x ld = %.2e elements: forward max |err| / bound %.3f, backward %.3f (bound 1)' % (rows * ld, e, e2))
    assert e <= 1.0 and e2 <= 1.0 and torch.equal(big.view(rows, ld)[-1, c:c + 64].view(torch.int16), tail_before.view(torch.int16))
