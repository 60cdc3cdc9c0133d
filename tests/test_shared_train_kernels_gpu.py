"""The kernels that four train engines share, each against a plain high-precision reference of the same operation on the MI355X:
rart_layernorm_bwd_full_bf16 and rart_colsum_bf16 (csrc/vit_bwd.hip; the LayerNorm's load, statistics and dx write are
csrc/rart_row_norm.h's, shared with csrc/row_norm.hip) against fp64 of the same bf16 operands, and the glue kernels
every engine runs (rart_engine_avgpool[_bwd][_pair], rart_f32_to_bf16_rows, rart_f32_to_pair_rows: csrc/engine_aux.hip, one kernel text
per operation for bf16 and pair storage; rart_vit_transpose_v, rart_vit_add_pos_cls).  The step kernels' share is in tests/test_train_steps_gpu.py.

Conventions: operands are bf16 and the reference is fp64 of those values; whatever a kernel must not read is NaN / +-inf, whatever it
must not write holds a sentinel (the workspace is filled with NaN bytes, so a partial sum that is read without having been written
shows); every launch is repeated and must be bit-identical; accumulate = 1 onto a random fp32 output equals pre + (accumulate = 0) exactly.

Bars (U = 2^-24; the right-hand sides in fp64):
  * LayerNorm dbeta, per column: |got - ref| <= (R_w + 1) U sum_r |dy|.  W = 4 min(ceil(rows / 4), 128) waves are launched and wave w
    walks rows w, w + W, ...: at most R_w = ceil(rows / W) bf16 terms per fp32 sum; the cross-wave sum is in double, rounded once.
  * LayerNorm dgamma, per column: |got - ref| <= (R_w + 2) U sum_r |dy xhat| + eps_hat sum_r |dy|.  eps_hat bounds the fp32 error of
    xhat; it comes from the reference alone: the same formula evaluated op by op in fp32 with torch, max |xhat_fp32 - xhat_fp64| over
    the case, times 4 (another summation order, a 2-ulp rsqrtf).
  * LayerNorm dx: the tolerance test_vit_backward_kernels gives rart_layernorm_bwd_bf16 (atol 3e-2, rtol 2e-2).
  * column sums: |got - ref| <= (rows_per_chunk + 1) U sum_r |x|, chunks = workspace bytes / (4 cols).
  * each of the bounds above must be able to fail: the fp64 reference without its last row, and without one wave's rows (every W-th
    row; column sums: without the last chunk that holds a row), lies outside the bound in >= 90 % of the columns.  Inputs are kept
    away from zero (|dy|, |x| >= 0.5) so that this is a property of the case and not of the draw.
  * pools: bf16 within one bf16 ulp of the fp64 value (+ hw U mean|x| for the forward's fp32 sum); pairs within 2^-16 |ref| plus the
    same slack; the backward exactly +0 wherever y <= 0.  Converters, the transpose and the position add: bit-exact.

No train engine passes the same buffer as dx and as res or dy (ViT and Mixer alternate two buffers, ConvNeXt passes no res), so no
aliased layout is tested; the layouts are the padded one, the engines' dense one, and ViT's final norm over the class tokens.

Measured on the MI355X, worst |err| / bound over the columns of a case (eps_hat as defined above, the factor 4 included):
  LayerNorm dgamma  dim  768: rows 1 0.2033 (eps_hat 1.40e-06)   rows 5 0.0826 (1.00e-06)   rows 511 0.0042 (2.19e-06)
                              rows 512 0.0052 (1.95e-06)   rows 513 0.0033 (2.66e-06)   rows 1300 0.0024 (2.59e-06)
                              class tokens (rows 3, x stride 197 * 768) 0.1485 (1.32e-06)
                    dim    8: rows 5 0.0430 (6.54e-07)   rows 513 0.0048 (1.06e-06)   rows 1300 0.0026 (1.29e-06)
                    dim  128: rows 1 0.1277 (6.87e-07)   rows 512 0.0060 (1.47e-06)   rows 1300 0.0029 (1.69e-06)
                    dim 1024: rows 5 0.0811 (1.31e-06)   rows 511 0.0047 (2.19e-06)   rows 1300 0.0030 (2.00e-06)
  LayerNorm dbeta and the column sums: 0.0000 in every case.  These inputs have 8 significant bits and a wave or a chunk adds at most
    127 of them, so every fp32 partial sum is exact and only the last rounding is left; the bound is what a change of the
    accumulation would have to respect, and what the mutilated references are measured against.
  LayerNorm dx: worst |err| / (3e-2 + 2e-2 |ref|) 0.111.  The mutilated references lie outside the bound in 99.6 % .. 100 % of the
    columns (LayerNorm) and in 98.4 % .. 100 % (column sums).
  pools, worst |err| / bound: bf16 forward 0.4990, backward 0.4898; pair forward 0.3130, backward 0.4882 (all 0 at hw = 1)"""
import numpy as np
import pytest
import torch

from test_mixer_gpu import _split, _ulp_bf16

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
EPS = 1e-6
NAN = float('nan')
SENT = 777.0                                        # exact in bf16 and fp32


def _lib():
    from robustart_amd import _lib as L
    return L, L.load()


def _bits(t):
    """the 16-bit patterns of a bf16 tensor"""
    return t.contiguous().view(torch.int16)


def _away_from_zero(shape, gen):
    v = torch.randn(shape, generator=gen)
    return torch.where(v >= 0, 0.5 + v, -0.5 + v)


def _workspace(need):
    return torch.full((max(need, 1),), 255, dtype=torch.uint8, device='cuda')           # NaN as fp32


# ------------------------------------------------------------------ rart_layernorm_bwd_full_bf16
def _ln_waves(rows):
    """the waves the host launches (vit_bwd.hip): four per workgroup, ceil(rows / 4) workgroups, at most 128 of them"""
    return 4 * min((rows + 3) // 4, 128)


def _ln_data(rows, dim, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, dim, generator=g) * 2 + 0.3).to(torch.bfloat16)
    dy = _away_from_zero((rows, dim), g).to(torch.bfloat16)
    res = torch.randn(rows, dim, generator=g).to(torch.bfloat16)
    gamma = 1 + 0.1 * torch.randn(dim, generator=g)
    return x, dy, res, gamma


def _ln_ref(x, dy, gamma):
    """fp64 of the same bf16 operands (biased variance, eps 1e-6)"""
    xd, dyd = x.double(), dy.double()
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (xd - mean) * rstd
    g = dyd * gamma.double()
    dx = rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    return {'xhat': xhat, 'dyx': dyd * xhat, 'dy': dyd, 'dx': dx}


def _xhat_fp32(x):
    """the same statistics op by op in fp32 with torch: the yardstick for eps_hat"""
    xf = x.float()
    d = xf.shape[1]
    t = xf - xf.sum(1, keepdim=True) / d
    return t * torch.rsqrt((t * t).sum(1, keepdim=True) / d + EPS)


def _ln_bounds(ref, x, rows):
    rw = -(-rows // _ln_waves(rows))
    eps_hat = 4.0 * (_xhat_fp32(x).double() - ref['xhat']).abs().max().item()
    mag_b = ref['dy'].abs().sum(0)
    return (rw + 2) * U32 * ref['dyx'].abs().sum(0) + eps_hat * mag_b, (rw + 1) * U32 * mag_b, eps_hat


def _ln_bound_can_fail(ref, bound_g, bound_b, rows):
    """the reference without its last row, and without every W-th row (one wave's), lies outside the bound in >= 90 % of the columns"""
    r = torch.arange(rows, device=ref['dy'].device)
    worst = 1.0
    for keep in (r < rows - 1, r % _ln_waves(rows) != 0):
        assert not keep.all()
        for terms, bound in ((ref['dyx'], bound_g), (ref['dy'], bound_b)):
            outside = ((terms[keep].sum(0) - terms.sum(0)).abs() > bound).double().mean().item()
            worst = min(worst, outside)
            assert outside >= 0.9, 'a mutilated reference lies inside the bound in %.1f %% of the columns' % (100 - 100 * outside)
    return worst


def _padded(t, stride, poison=NAN):
    """device bf16 [rows][stride]: t in the leading columns, `poison` in the slack"""
    buf = torch.full((t.shape[0], stride), poison, dtype=torch.bfloat16)
    buf[:, :t.shape[1]] = t
    return buf.cuda()


def _ln_launch(dy, x, gamma, res, dx, rows, dim, strides, out, accumulate=0, short=0):
    """out: fp32 [2][dim + 8], dgamma and dbeta in the leading dim columns; -> the status"""
    L, lib = _lib()
    need = lib.rart_layernorm_bwd_workspace_bytes(dim)
    ws = _workspace(need)
    return lib.rart_layernorm_bwd_full_bf16(L.ptr(dy), L.ptr(x), L.ptr(gamma), L.ptr(res), L.ptr(dx), rows, dim, strides[0], strides[1],
                                            strides[2], strides[3], EPS, L.ptr(out[0]), L.ptr(out[1]), accumulate, L.ptr(ws),
                                            need - short, L.stream_ptr())


def _ln_out(dim, pre=None):
    out = torch.full((2, dim + 8), SENT, device='cuda')
    out[:, :dim] = NAN if pre is None else pre
    return out


def _ln_check_dx(dxb, want, dim):
    got = dxb[:, :dim].double()
    assert torch.isfinite(got).all()
    ratio = ((got - want).abs() / (3e-2 + 2e-2 * want.abs())).max().item()
    assert ratio <= 1.0, 'dx: worst |err| / tolerance %.3f' % ratio
    assert (dxb[:, dim:] == SENT).all()                                  # the slack of dx is not written
    return ratio


LN_CASES = [(768, r) for r in (1, 5, 511, 512, 513, 1300)] + [(8, r) for r in (5, 513, 1300)] + \
           [(128, r) for r in (1, 512, 1300)] + [(1024, r) for r in (5, 511, 1300)]


@pytest.mark.parametrize('dim,rows', LN_CASES)
def test_layernorm_bwd_full_vs_fp64(dim, rows):
    """padded, unequal row strides with NaN in the slack; res null and non-null; dx null; accumulate; a short workspace"""
    L, lib = _lib()
    x, dy, res, gamma = _ln_data(rows, dim, 1000 * dim + rows)
    strides = (dim + 8, dim + 16, dim + 24, dim + 32)
    dyb, xb, rb, gam = _padded(dy, strides[0]), _padded(x, strides[1]), _padded(res, strides[2]), gamma.cuda()
    ref = _ln_ref(x.cuda(), dy.cuda(), gam)
    bound_g, bound_b, eps_hat = _ln_bounds(ref, x.cuda(), rows)
    ref_g, ref_b = ref['dyx'].sum(0), ref['dy'].sum(0)
    outside = _ln_bound_can_fail(ref, bound_g, bound_b, rows) if rows >= 5 else None

    def run(res_buf, with_dx=True, pre=None):
        out = _ln_out(dim, pre)
        dxb = torch.full((rows, strides[3]), SENT, dtype=torch.bfloat16, device='cuda') if with_dx else None
        L.check(_ln_launch(dyb, xb, gam, res_buf, dxb, rows, dim, strides, out, accumulate=0 if pre is None else 1))
        assert (out[:, dim:] == SENT).all()
        return out[:, :dim], dxb

    got, dxb = run(None)
    assert torch.isfinite(got).all()
    ratio_g = ((got[0].double() - ref_g).abs() / bound_g).max().item()
    ratio_b = ((got[1].double() - ref_b).abs() / bound_b).max().item()
    ratio_x = _ln_check_dx(dxb, ref['dx'], dim)
    print('layernorm_bwd_full dim %d rows %d (W %d): worst |err| / bound dgamma %.4f dbeta %.4f, eps_hat %.2e, dx |err| / tolerance %.3f%s'
          % (dim, rows, _ln_waves(rows), ratio_g, ratio_b, eps_hat, ratio_x,
             '' if outside is None else ', mutilated references outside the bound in >= %.1f %% of the columns' % (100 * outside)))
    assert ratio_g <= 1.0 and ratio_b <= 1.0
    again, dxb2 = run(None)
    assert torch.equal(got, again) and torch.equal(_bits(dxb), _bits(dxb2)), 'second run differs'
    with_res, dxr = run(rb)
    assert torch.equal(got, with_res)                                    # res reaches dx alone
    _ln_check_dx(dxr, ref['dx'] + res.cuda().double(), dim)
    no_dx, _ = run(None, with_dx=False)
    assert torch.equal(got, no_dx)                                       # dx is optional, the sums do not depend on it
    pre = torch.randn(2, dim, generator=torch.Generator().manual_seed(rows)).cuda()
    acc, _ = run(rb, pre=pre)
    assert torch.equal(acc, pre + got), 'accumulate'
    # a workspace one byte short is refused and nothing is written
    out, dxs = _ln_out(dim), torch.full((rows, strides[3]), SENT, dtype=torch.bfloat16, device='cuda')
    assert _ln_launch(dyb, xb, gam, rb, dxs, rows, dim, strides, out, short=1) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out[:, :dim]).all() and (out[:, dim:] == SENT).all() and (dxs == SENT).all()


def test_layernorm_bwd_full_engine_layouts():
    """the engines' own calls: dense rows with a residual (every block norm), and ViT's final norm over the class tokens, whose rows lie
    197 * 768 elements apart in x and in dx while dy is dense"""
    L, lib = _lib()
    D, T, B = 768, 197, 3
    # dense, res non-null: _ln_bwd_full(dln, xm, gamma, dx, dxm, rows, (D, D, D, D))
    rows = 37
    x, dy, res, gamma = _ln_data(rows, D, 5)
    gam = gamma.cuda()
    ref = _ln_ref(x.cuda(), dy.cuda(), gam)
    bound_g, bound_b, _ = _ln_bounds(ref, x.cuda(), rows)
    _ln_bound_can_fail(ref, bound_g, bound_b, rows)
    out, dxb = _ln_out(D), torch.full((rows, D), SENT, dtype=torch.bfloat16, device='cuda')
    L.check(_ln_launch(dy.cuda(), x.cuda(), gam, res.cuda(), dxb, rows, D, (D, D, D, D), out))
    assert ((out[0, :D].double() - ref['dyx'].sum(0)).abs() <= bound_g).all()
    assert ((out[1, :D].double() - ref['dy'].sum(0)).abs() <= bound_b).all()
    _ln_check_dx(dxb, ref['dx'] + res.cuda().double(), D)
    # class tokens: _ln_bwd_full(dcls, x_last, gamma, None, dx, B, (D, T * D, 0, T * D))
    x, dy, _, gamma = _ln_data(B, D, 6)
    gam = gamma.cuda()
    xb = torch.full((B, T, D), NAN, dtype=torch.bfloat16)
    xb[:, 0] = x
    xb = xb.cuda()
    ref = _ln_ref(x.cuda(), dy.cuda(), gam)
    bound_g, bound_b, eps_hat = _ln_bounds(ref, x.cuda(), B)
    got = []
    for _ in range(2):
        out, dxb = _ln_out(D), torch.full((B, T, D), SENT, dtype=torch.bfloat16, device='cuda')
        L.check(_ln_launch(dy.cuda(), xb, gam, None, dxb, B, D, (D, T * D, 0, T * D), out))
        assert (out[:, D:] == SENT).all() and (dxb[:, 1:] == SENT).all()          # the other tokens' gradients are not touched
        _ln_check_dx(dxb[:, 0], ref['dx'], D)
        got.append((out, dxb))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(_bits(got[0][1]), _bits(got[1][1]))
    ratio_g = ((got[0][0][0, :D].double() - ref['dyx'].sum(0)).abs() / bound_g).max().item()
    ratio_b = ((got[0][0][1, :D].double() - ref['dy'].sum(0)).abs() / bound_b).max().item()
    print('layernorm_bwd_full class tokens (rows %d, x stride %d): worst |err| / bound dgamma %.4f dbeta %.4f, eps_hat %.2e'
          % (B, T * D, ratio_g, ratio_b, eps_hat))
    assert ratio_g <= 1.0 and ratio_b <= 1.0


# ------------------------------------------------------------------ rart_colsum_bf16
# (rows, cols, ld, chunks): one chunk; the first split; uneven chunks; 2 056 columns = one 8-column vector past a workgroup of 256
# vectors; the 256-chunk cap; 16 450 rows = 65 per chunk, so chunks 254 and 255 hold no row; ViT's position embedding (ld = cols)
COLSUM_CASES = [(1, 8, 8, 1), (127, 768, 784, 1), (128, 768, 768, 2), (191, 2056, 2064, 2), (191, 768, 776, 2), (16384, 8, 16, 256),
                (16450, 64, 72, 256), (2, 151296, 151296, 1)]


def _colsum_launch(xb, ld, rows, cols, out, accumulate=0, short=0):
    L, lib = _lib()
    need = lib.rart_colsum_workspace_bytes(rows, cols)
    ws = _workspace(need)
    return lib.rart_colsum_bf16(L.ptr(xb), ld, rows, cols, L.ptr(out), accumulate, L.ptr(ws), need - short, L.stream_ptr()), need // (4 * cols)


@pytest.mark.parametrize('rows,cols,ld,chunks', COLSUM_CASES, ids=lambda v: str(v))
def test_colsum_vs_fp64(rows, cols, ld, chunks):
    L, lib = _lib()
    g = torch.Generator().manual_seed(rows + 7 * cols)
    x = _away_from_zero((rows, cols), g).to(torch.bfloat16)
    xb = torch.full((rows, ld), NAN, dtype=torch.bfloat16)
    xb[:, cols::3] = float('inf')
    xb[:, cols + 1::3] = float('-inf')
    xb[:, :cols] = x
    xb = xb.cuda()
    xd = x.cuda().double()
    ref, mag = xd.sum(0), xd.abs().sum(0)

    def run(pre=None, short=0):
        out = torch.full((cols + 8,), SENT, device='cuda')
        out[:cols] = NAN if pre is None else pre
        st, n_chunks = _colsum_launch(xb, ld, rows, cols, out, accumulate=0 if pre is None else 1, short=short)
        return st, n_chunks, out

    st, n_chunks, out = run()
    L.check(st)
    assert n_chunks == chunks
    per = -(-rows // n_chunks)
    bound = (per + 1) * U32 * mag
    if rows >= 5:           # without the last row; without the last chunk that holds a row
        r = torch.arange(rows, device='cuda')
        for keep in (r < rows - 1, r < (rows - 1) // per * per):
            outside = ((xd[keep].sum(0) - ref).abs() > bound).double().mean().item()
            assert outside >= 0.9, 'a mutilated reference lies inside the bound in %.1f %% of the columns' % (100 - 100 * outside)
    got = out[:cols]
    assert torch.isfinite(got).all() and (out[cols:] == SENT).all()
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print('colsum %d x %d (ld %d, %d chunks of %d rows): worst |err| / bound = %.4f' % (rows, cols, ld, n_chunks, per, ratio))
    assert ratio <= 1.0
    assert torch.equal(run()[2], out), 'second run differs'
    pre = torch.randn(cols, generator=g).cuda()
    st, _, acc = run(pre=pre)
    L.check(st)
    assert torch.equal(acc[:cols], pre + got) and (acc[cols:] == SENT).all(), 'accumulate'
    st, _, out = run(short=1)
    torch.cuda.synchronize()
    assert st != 0 and torch.isnan(out[:cols]).all() and (out[cols:] == SENT).all()        # a short workspace is refused


# ------------------------------------------------------------------ global average pool, bf16 and pair
POOL_SHAPES = [(1, 1, 8), (3, 49, 2048), (2, 196, 768)]


def _pool_y(n, hw, c, gen):
    """the pool's input as the backward sees it: +0.0, -0.0 and negative values among the positive ones"""
    y = torch.randn(n, hw, c, generator=gen)
    y.view(-1)[0::7] = 0.0
    y.view(-1)[1::7] = -0.0
    y.view(-1)[2::7] = -1.5
    return y


@pytest.mark.parametrize('n,hw,c', POOL_SHAPES)
def test_avgpool_bf16_forward_and_backward(n, hw, c):
    L, lib = _lib()
    sp = L.stream_ptr()
    g = torch.Generator().manual_seed(hw + c)
    x = torch.randn(n, hw, c, generator=g).to(torch.bfloat16).cuda()
    outs = []
    for _ in range(2):
        out = torch.full((n, c), NAN, dtype=torch.bfloat16, device='cuda')
        L.check(lib.rart_engine_avgpool(L.ptr(x), L.ptr(out), n, hw, c, sp))
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    xd = x.double()
    ref = xd.mean(1)
    fwd = ((outs[0].double() - ref).abs() / (_ulp_bf16(ref) + hw * U32 * xd.abs().mean(1))).max().item()
    y = _pool_y(n, hw, c, g).to(torch.bfloat16).cuda()
    dpool = torch.randn(n, c, generator=g).to(torch.bfloat16).cuda()
    dzs = []
    for _ in range(2):
        dz = torch.full((n, hw, c), NAN, dtype=torch.bfloat16, device='cuda')
        L.check(lib.rart_engine_avgpool_bwd(L.ptr(y), L.ptr(dpool), L.ptr(dz), n, hw, c, sp))
        dzs.append(dz)
    assert torch.equal(_bits(dzs[0]), _bits(dzs[1]))
    want = (dpool.double() / hw)[:, None, :].expand(n, hw, c)
    live = y > 0
    assert live.any() and not live.all()
    bwd = ((dzs[0].double() - want).abs() / _ulp_bf16(want))[live].max().item()
    print('avgpool bf16 %s: forward worst |err| / (ulp + hw U mean|x|) = %.4f, backward worst |err| / ulp = %.4f' % ((n, hw, c), fwd, bwd))
    assert fwd <= 1.0 and bwd <= 1.0
    assert (_bits(dzs[0])[~live] == 0).all()                              # exactly +0 wherever y <= 0 (+0.0, -0.0, negative)


@pytest.mark.parametrize('n,hw,c', POOL_SHAPES)
def test_avgpool_pair_forward_and_backward(n, hw, c):
    L, lib = _lib()
    sp = L.stream_ptr()
    g = torch.Generator().manual_seed(3 * hw + c)
    x = _split(torch.randn(n, hw, c, generator=g)).cuda()               # [2][n][hw][c]: the lo plane numel() elements behind hi
    outs = []
    for _ in range(2):
        out = torch.full((2, n, c), NAN, dtype=torch.bfloat16, device='cuda')
        L.check(lib.rart_engine_avgpool_pair(L.ptr(x), x[0].numel(), L.ptr(out), out[0].numel(), n, hw, c, sp))
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    xd = x[0].double() + x[1].double()
    ref = xd.mean(1)
    fwd = ((outs[0][0].double() + outs[0][1].double() - ref).abs() / (2.0 ** -16 * ref.abs() + hw * U32 * xd.abs().mean(1))).max().item()
    # the 1-bit (y > 0) operand: uint8 [n][hw][c / 8], bit j of byte k = channel 8k + j > 0
    live = _pool_y(n, hw, c, g) > 0
    sign = (live.view(n, hw, c // 8, 8).int() * (2 ** torch.arange(8, dtype=torch.int32))).sum(-1).to(torch.uint8).cuda()
    live = live.cuda()
    dpool = _split(torch.randn(n, c, generator=g)).cuda()
    dzs = []
    for _ in range(2):
        dz = torch.full((2, n, hw, c), NAN, dtype=torch.bfloat16, device='cuda')
        L.check(lib.rart_engine_avgpool_bwd_pair(L.ptr(sign), L.ptr(dpool), dpool[0].numel(), L.ptr(dz), dz[0].numel(), n, hw, c, sp))
        dzs.append(dz)
    assert torch.equal(_bits(dzs[0]), _bits(dzs[1]))
    want = ((dpool[0].double() + dpool[1].double()) / hw)[:, None, :].expand(n, hw, c)
    bwd = ((dzs[0][0].double() + dzs[0][1].double() - want).abs() / (2.0 ** -16 * want.abs()))[live].max().item()
    print('avgpool pair %s: forward worst |err| / (2^-16 |ref| + hw U mean|x|) = %.4f, backward worst |err| / (2^-16 |ref|) = %.4f'
          % ((n, hw, c), fwd, bwd))
    assert fwd <= 1.0 and bwd <= 1.0
    assert (_bits(dzs[0][0])[~live] == 0).all() and (_bits(dzs[0][1])[~live] == 0).all()


# ------------------------------------------------------------------ fp32 rows -> bf16 / pair rows
# +-0, fp32 and bf16 subnormals (0x00008000 and 0x00018000 lie half-way between two bf16 subnormals), half-way cases of both
# parities and both signs with their neighbours, and the values around the largest finite bf16 that still round to it
SPECIAL_BITS = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x0000FFFF, 0x007FFFFF, 0x807FFFFF,
                0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,
                0x7F7EFFFF, 0x7F7F0000, 0x7F7F7FFF, 0xFF7F7FFF]
ROW_SHAPES = [(1, 1, 8), (4, 1000, 1024), (3, 63, 64)]


def _rows_src(rows, cols):
    src = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols))
    special = torch.from_numpy(np.array(SPECIAL_BITS, dtype=np.uint32).view(np.float32).copy())
    if cols >= len(SPECIAL_BITS):
        for r in range(rows):
            src[r, r:r + len(SPECIAL_BITS)] = special                   # at another column parity in every row
    else:
        src[0, 0] = special[10]                                          # 0x3F818000: half-way, rounds up to the even neighbour
    return src


@pytest.mark.parametrize('rows,cols,dst_cols', ROW_SHAPES)
def test_f32_to_bf16_rows_bit_exact(rows, cols, dst_cols):
    L, lib = _lib()
    src = _rows_src(rows, cols)
    want = torch.zeros(rows, dst_cols, dtype=torch.bfloat16)
    want[:, :cols] = src.to(torch.bfloat16)
    src_d, dst = src.cuda(), torch.full((rows, dst_cols), NAN, dtype=torch.bfloat16, device='cuda')
    L.check(lib.rart_f32_to_bf16_rows(L.ptr(src_d), L.ptr(dst), rows, cols, dst_cols, L.stream_ptr()))
    assert torch.equal(_bits(dst).cpu(), _bits(want))                    # the padding columns exactly +0


@pytest.mark.parametrize('rows,cols,dst_cols', ROW_SHAPES)
def test_f32_to_pair_rows_bit_exact(rows, cols, dst_cols):
    L, lib = _lib()
    src = _rows_src(rows, cols)
    want = torch.zeros(2, rows, dst_cols, dtype=torch.bfloat16)
    want[:, :, :cols] = _split(src)
    src_d, dst = src.cuda(), torch.full((2, rows, dst_cols), NAN, dtype=torch.bfloat16, device='cuda')
    L.check(lib.rart_f32_to_pair_rows(L.ptr(src_d), L.ptr(dst), dst[0].numel(), rows, cols, dst_cols, L.stream_ptr()))
    assert torch.equal(_bits(dst).cpu(), _bits(want))                    # the padding of both planes exactly +0


# ------------------------------------------------------------------ ViT glue
@pytest.mark.parametrize('heads', [1, 12])
@pytest.mark.parametrize('B', [1, 3])
def test_vit_transpose_v_bit_exact(B, heads):
    """vt[b][h][d][t] = qkv[b][t][v_off + 64 h + d], zeros in t >= T: every (qkv_ld, v_off) the engines pass (V, K, Q of the fused
    activation, and the dense attention-output gradient)"""
    L, lib = _lib()
    D, tail = heads * 64, 64
    g = torch.Generator().manual_seed(B + heads)
    for T in (196, 197):
        for t_pad in (200, 224):
            for ld, off in ((3 * D, 0), (3 * D, D), (3 * D, 2 * D), (D, 0)):
                src = torch.randint(-32768, 32768, (B, T, ld), generator=g, dtype=torch.int32).to(torch.int16).cuda()   # any bit pattern
                n = B * heads * 64 * t_pad
                vt = torch.full((n + tail,), NAN, dtype=torch.bfloat16, device='cuda')
                L.check(lib.rart_vit_transpose_v(L.ptr(src), L.ptr(vt), B, T, heads, 64, ld, off, t_pad, L.stream_ptr()))
                want = torch.zeros(B, heads, 64, t_pad, dtype=torch.int16, device='cuda')
                want[..., :T] = src[:, :, off:off + D].view(B, T, heads, 64).permute(0, 2, 3, 1)
                assert torch.equal(_bits(vt[:n]).view(B, heads, 64, t_pad), want), (T, t_pad, ld, off)
                assert torch.isnan(vt[n:]).all()


@pytest.mark.parametrize('B', [1, 3])
def test_vit_add_pos_cls_bf16_bit_exact(B):
    L, lib = _lib()
    T, D = 197, 768
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, T, D, generator=g).to(torch.bfloat16)
    x[:, 0] = NAN                                                        # whatever the class-token slot held is replaced
    cls_pos0 = torch.randn(D, generator=g)
    pos = 0.5 * torch.randn(T, D, generator=g)
    pos[0] = NAN                                                         # row 0 of pos is not read: cls_pos0 already holds it
    want = (x.float() + pos).to(torch.bfloat16)
    want[:, 0] = cls_pos0.to(torch.bfloat16)
    xg, cls_d, pos_d = x.cuda(), cls_pos0.cuda(), pos.cuda()
    L.check(lib.rart_vit_add_pos_cls(L.ptr(xg), L.ptr(cls_d), L.ptr(pos_d), B, T, D, L.stream_ptr()))
    assert torch.equal(_bits(xg).cpu(), _bits(want))
