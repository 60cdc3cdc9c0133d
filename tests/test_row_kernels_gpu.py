"""The plain row kernels every engine calls through engine_base.py (_rows, _ln, _ln_bwd, _fc1_gelu), each against the fp64
reference of the same operation on the MI355X: rart_layernorm[_bwd]_{bf16,pair}, rart_softmax[_bwd]_rows_{bf16,pair},
rart_gelu[_bwd]_bf16 (LayerNorm: csrc/row_norm.hip, one kernel per direction for both storages; soft-max: csrc/vit_aux.hip,
csrc/vit_bwd.hip, csrc/vit_pair.hip; GELU: csrc/vit_bwd.hip).  References, inputs and bounds are in
tests/_row_kernels_ref.py; tests/test_row_kernel_refs_cpu.py shows on the CPU that a plain fp32 implementation meets the bounds
and that the listed wrong ones do not.

Conventions: calls go through robustart_amd._lib and the status is checked; every launch is run twice into fresh buffers and must
be bit-identical; every output buffer is pre-filled with the bf16 bit pattern 0x7FA5, a NaN no result can be, with GUARD_ROWS rows
(GELU: TAIL elements) behind what the call names, and every element the contract does not name must still hold it afterwards (rows
past `rows`; LayerNorm: columns from dim to the output stride; the other token rows of the ViT head's layouts); every slack element
of an input is NaN.

LayerNorm: dims 8 .. 1024 on either side of every vector-slot boundary, rows on either side of the four-rows-per-workgroup
boundary, dense and padded strides, the ViT head's class-token strides, backward with and without the residual; the planted rows
of R.rows_for: (b) comes out as the stored form of beta exactly, (e) bit-identical to row 0.  eps = 1e-6 throughout: no caller
passes another value to these entries (1e-5 is rart_ln_gelu's).  Soft-max: n_valid / leading dimensions at both ends of the lane
layout, NaN slack, zeros in the output's slack, rows summing to 1.  GELU: every bf16 operand of R.gelu_patterns, ragged sizes, and
sizes past one grid trip, where every element must equal the exhaustive case's output for the same pattern.  The size the issue
names for that, 8 (2048 * 256 + 3), is rart_grid_for's DEFAULT cap; k_gelu's grid_for passes 256 * 16 workgroups, so that size is
2049 workgroups in one trip, and 8 (R.GELU_GRID_ITEMS + 3) is the size that takes the second trip.  Both run.

Every test prints its worst |err| / bound and the module's worst so far for that kernel.  Measured on the MI355X, worst over all
cases, beside the fp32 mirror's figure from the CPU test:
  kernel                       MI355X   mirror        kernel                        MI355X   mirror
  rart_layernorm_bf16          0.4935   0.4935        rart_layernorm_pair           0.1295   0.1295
  rart_layernorm_bwd_bf16      0.4925   0.4925        rart_layernorm_bwd_pair       0.4370   0.4370
  rart_softmax_rows_bf16       0.4765   0.4765        rart_softmax_rows_pair        0.1840   0.1840
  rart_softmax_bwd_rows_bf16   0.4895   0.4895        rart_softmax_bwd_rows_pair    0.2248   0.2248
  rart_gelu_bf16               0.4876   0.4876        rart_gelu_bwd_bf16            0.4967   0.4967
(the worst element of each is decided by the rounding of the stored result, which the kernel and the mirror share).  Every exact
check holds.  Against a build of the sources with ten deliberate, memory-safe mistakes, made when the bf16 and the pair kernels were
still separate copies (variance / (d - 1) in what is now k_layernorm<false>, the mean without slot 1 in k_layernorm_bwd<false>, eps
outside the root in k_layernorm<true>, no xhat term in k_layernorm_bwd<true>, <= n_valid
in both soft-max forwards, the mask multiplied in instead of selected in k_softmax_bwd_rows, the dot over ld_p in
k_softmax_bwd_rows_pair, tanh GELU, GELU' without v phi, a grid stride one too long in k_gelu) 114 of the 137 cases fail; the 23
that pass are the ones those mistakes do not reach: the eight soft-max cases without slack columns, the thirteen bf16 LayerNorm
backward cases at dims that end in slot 0, the pair LayerNorm forward without planted rows (eps does not matter there), and the
GELU size of one grid trip, which is compared with the exhaustive output."""
import pytest
import torch

import _row_kernels_ref as R

pytestmark = pytest.mark.gpu

PRECS = ('bf16', 'pair')
SENT = 0x7FA5                                       # a bf16 NaN
GUARD_ROWS = 3
TAIL = 64
LN_IDS = ['%dx%d' % s for s in R.LN_SHAPES]
_worst = {}


def _lib():
    from robustart_amd import _lib as L
    return L, L.load()


def _note(name, case, ratio):
    _worst[name] = max(_worst.get(name, 0.0), ratio)
    print('%s %s: worst |err| / bound = %.4f (so far %.4f)' % (name, case, ratio, _worst[name]))
    return ratio


def _bits(t):
    return t.contiguous().view(torch.int16)


def _sentinel(*shape):
    return torch.full(shape, SENT, dtype=torch.int16, device='cuda').view(torch.bfloat16)


def _in_planes(v, prec, ld):
    """stored fp32 values [rows][cols] on the CPU -> the device planes [rows][ld], NaN from column cols on"""
    out = []
    for p in R.planes(v, prec):
        buf = torch.full((v.shape[0], ld), R.NAN, dtype=torch.bfloat16)
        buf[:, :v.shape[1]] = p
        out.append(buf.cuda())
    return out


def _in_f32(v, ld):
    buf = torch.full((v.shape[0], ld), R.NAN, dtype=torch.float32)
    buf[:, :v.shape[1]] = v
    return buf.cuda()


def _out_planes(rows, ld, prec):
    return [_sentinel(rows + GUARD_ROWS, ld) for _ in range(1 if prec == 'bf16' else 2)]


def _ptrs(L, pl):
    return [L.ptr(p) for p in pl]


def _named(pl, rows, cols):
    """-> the planes' [rows][cols] corner on the CPU; everything else must still be the sentinel"""
    got = []
    for p in pl:
        b = _bits(p).cpu()
        rest = torch.ones_like(b, dtype=torch.bool)
        rest[:rows, :cols] = False
        assert (b[rest] == SENT).all(), 'written outside the contract'
        got.append(p.cpu()[:rows, :cols])
    return got


def _same_bits(a, b):
    return all(torch.equal(_bits(s), _bits(t)) for s, t in zip(a, b))


def _twice(run):
    a, b = run(), run()
    torch.cuda.synchronize()
    assert _same_bits(a, b), 'second launch differs'
    return a


# ------------------------------------------------------------------ LayerNorm
def _ln_fwd(prec, c, x, rows, dim, ld_in, ld_out):
    """x: stored fp32 [rows][dim] -> the output planes [rows][dim] on the CPU"""
    L, lib = _lib()
    xd, g, b = _in_planes(x, prec, ld_in), c['gamma'].cuda(), c['beta'].cuda()
    fn = lib.rart_layernorm_bf16 if prec == 'bf16' else lib.rart_layernorm_pair

    def run():
        out = _out_planes(rows, ld_out, prec)
        L.check(fn(*_ptrs(L, xd), L.ptr(g), L.ptr(b), *_ptrs(L, out), rows, dim, ld_in, ld_out, R.EPS, L.stream_ptr()))
        return out
    return _named(_twice(run), rows, dim)


def _ln_bwd(prec, c, x, dy, res, rows, dim, strides):
    """strides: the row strides of (dy, x, res, dx); res None goes in as null pointers"""
    L, lib = _lib()
    s_dy, s_x, s_res, s_dx = strides
    dyd, xd, g = _in_planes(dy, prec, s_dy), _in_planes(x, prec, s_x), c['gamma'].cuda()
    rd = [None] * len(xd) if res is None else _in_planes(res, prec, s_res)
    fn = lib.rart_layernorm_bwd_bf16 if prec == 'bf16' else lib.rart_layernorm_bwd_pair

    def run():
        out = _out_planes(rows, s_dx, prec)
        L.check(fn(*_ptrs(L, dyd), *_ptrs(L, xd), L.ptr(g), *_ptrs(L, rd), *_ptrs(L, out), rows, dim, s_dy, s_x, s_res, s_dx, R.EPS,
                   L.stream_ptr()))
        return out
    return _named(_twice(run), rows, dim)


def _ln_layouts(dim):
    return (('dense', dim), ('padded', dim + 8))


@pytest.mark.parametrize('shape', R.LN_SHAPES, ids=LN_IDS)
@pytest.mark.parametrize('prec', PRECS)
def test_layernorm_forward(prec, shape):
    rows, dim = shape
    c = R.ln_case(rows, dim, prec)
    ref = R.ln_fwd_ref(c['x'], c['gamma'], c['beta'])
    bound, _ = R.ln_fwd_bound(c['x'], c['gamma'], c['beta'], prec)
    for name, ld in _ln_layouts(dim):
        got = _ln_fwd(prec, c, c['x'], rows, dim, ld, ld)
        ratio = _note('layernorm_%s' % prec, '%s %s' % (shape, name), R.worst(R.value64(got) - ref, bound))
        assert ratio <= 1.0
        if c['planted']:
            assert _same_bits([p[R.ROW_B] for p in got], R.planes(c['beta'], prec)), 'row (b) is not the stored form of beta'
            assert _same_bits([p[rows - 1] for p in got], [p[0] for p in got]), 'row (e) differs from row 0'


@pytest.mark.parametrize('shape', R.LN_SHAPES, ids=LN_IDS)
@pytest.mark.parametrize('prec', PRECS)
def test_layernorm_backward(prec, shape):
    rows, dim = shape
    c = R.ln_case(rows, dim, prec)
    for res in (c['res'], None):
        ref = R.ln_bwd_ref(c['x'], c['dy'], c['gamma'], res)
        bound = R.ln_bwd_bound(c['x'], c['dy'], c['gamma'], res, prec)
        for name, ld in _ln_layouts(dim):
            got = _ln_bwd(prec, c, c['x'], c['dy'], res, rows, dim, (ld, ld, 0 if res is None else ld, ld))
            case = '%s %s %s' % (shape, name, 'no res' if res is None else 'res')
            assert _note('layernorm_bwd_%s' % prec, case, R.worst(R.value64(got) - ref, bound)) <= 1.0
            if c['planted']:
                assert _same_bits([p[rows - 1] for p in got], [p[0] for p in got]), 'row (e) differs from row 0'


@pytest.mark.parametrize('prec', PRECS)
def test_layernorm_vit_head_layouts(prec):
    """the class-token rows of [B][T][D]: forward ld_in = T D, ld_out = D; backward strides (D, T D, 0, T D) with res null.  The
    other T - 1 token rows are NaN in the inputs and must keep the sentinel in the backward's output"""
    B, T, D = R.HEAD_SHAPE
    c = R.ln_case(6, D, prec)
    x, dy = c['x'][:B], c['dy'][:B]
    ref = R.ln_fwd_ref(x, c['gamma'], c['beta'])
    bound, _ = R.ln_fwd_bound(x, c['gamma'], c['beta'], prec)
    got = _ln_fwd(prec, c, x, B, D, T * D, D)
    assert _note('layernorm_%s' % prec, 'head %s' % (R.HEAD_SHAPE,), R.worst(R.value64(got) - ref, bound)) <= 1.0
    ref = R.ln_bwd_ref(x, dy, c['gamma'], None)
    bound = R.ln_bwd_bound(x, dy, c['gamma'], None, prec)
    got = _ln_bwd(prec, c, x, dy, None, B, D, (D, T * D, 0, T * D))
    assert _note('layernorm_bwd_%s' % prec, 'head %s' % (R.HEAD_SHAPE,), R.worst(R.value64(got) - ref, bound)) <= 1.0


# ------------------------------------------------------------------ soft-max rows
def _sm_fwd(prec, s, rows, shape, scale):
    L, lib = _lib()
    n, ld_in, ld_out = shape
    sd = _in_planes(s, 'bf16', ld_in)[0] if prec == 'bf16' else _in_f32(s, ld_in)
    fn = lib.rart_softmax_rows_bf16 if prec == 'bf16' else lib.rart_softmax_rows_pair

    def run():
        out = _out_planes(rows, ld_out, prec)
        L.check(fn(L.ptr(sd), *_ptrs(L, out), rows, n, ld_in, ld_out, scale, L.stream_ptr()))
        return out
    return _named(_twice(run), rows, ld_out)


def _sm_bwd(prec, p, dp, rows, shape, scale):
    """(ld_p, ld_dp, ld_out) = the forward's (ld_out, ld_in, ld_out), as vit_engine.py calls it"""
    L, lib = _lib()
    n, ld_in, ld_out = shape
    pd = _in_planes(p, prec, ld_out)
    dpd = _in_planes(dp, 'bf16', ld_in)[0] if prec == 'bf16' else _in_f32(dp, ld_in)
    fn = lib.rart_softmax_bwd_rows_bf16 if prec == 'bf16' else lib.rart_softmax_bwd_rows_pair

    def run():
        out = _out_planes(rows, ld_out, prec)
        L.check(fn(*_ptrs(L, pd), L.ptr(dpd), *_ptrs(L, out), rows, n, ld_out, ld_in, ld_out, scale, L.stream_ptr()))
        return out
    return _named(_twice(run), rows, ld_out)


def _sm_params():
    return [pytest.param(prec, shape, rows, id='%s-%s-rows%d' % (prec, 'x'.join(map(str, shape)), rows)) for prec in PRECS
            for shape, rows in R.sm_cases(prec)]


@pytest.mark.parametrize('prec,shape,rows', _sm_params())
def test_softmax_forward(prec, shape, rows):
    n, ld_in, ld_out = shape
    for scale in R.SM_SCALES:
        c = R.sm_case(prec, shape, rows, scale)
        ref = R.sm_fwd_ref(c['s'], n, scale)
        got = R.value64(_sm_fwd(prec, c['s'], rows, shape, scale))
        assert not torch.isnan(got).any(), 'NaN in the output'
        assert (got[:, n:] == 0).all(), 'the output slack is not zero'
        assert (got.sum(-1) - 1).abs().max().item() <= ld_out * 2.0 ** -8
        case = '%s rows %d scale %g' % (shape, rows, scale)
        assert _note('softmax_rows_%s' % prec, case, R.worst(got[:, :n] - ref, R.sm_fwd_bound(ref, prec))) <= 1.0


@pytest.mark.parametrize('prec,shape,rows', _sm_params())
def test_softmax_backward(prec, shape, rows):
    n, ld_in, ld_out = shape
    for scale in R.SM_SCALES:
        c = R.sm_case(prec, shape, rows, scale)
        ref = R.sm_bwd_ref(c['p'], c['dp'], n, scale)
        bound = R.sm_bwd_bound(c['p'], c['dp'], n, scale, prec)
        got = R.value64(_sm_bwd(prec, c['p'][:, :n], c['dp'][:, :n], rows, shape, scale))
        assert not torch.isnan(got).any(), 'NaN in the output'
        assert (got[:, n:] == 0).all(), 'the output slack is not zero'
        case = '%s rows %d scale %g' % (shape, rows, scale)
        assert _note('softmax_bwd_rows_%s' % prec, case, R.worst(got[:, :n] - ref, bound)) <= 1.0


# ------------------------------------------------------------------ GELU
def _gelu(u, dh=None):
    """u (and dh) bf16 on the device, n = u.numel() -> the n outputs; the TAIL behind them must keep the sentinel"""
    L, lib = _lib()
    n = u.numel()

    def run():
        out = _sentinel(n + TAIL)
        if dh is None:
            L.check(lib.rart_gelu_bf16(L.ptr(u), L.ptr(out), n, L.stream_ptr()))
        else:
            L.check(lib.rart_gelu_bwd_bf16(L.ptr(dh), L.ptr(u), L.ptr(out), n, L.stream_ptr()))
        return (out,)
    out, = _twice(run)
    assert (_bits(out[n:]) == SENT).all(), 'written past n'
    return out[:n]


@pytest.fixture(scope='module')
def exhaustive():
    """the operand set on the device, its fp64 gelu and gelu', and the kernels' outputs for it (bwd: per dh)"""
    u, n = R.gelu_operands()
    y, dy = R.gelu_ref(u)
    ud = u.cuda()
    fwd = _gelu(ud)
    bwd = {dh: _gelu(ud, torch.full_like(ud, dh)) for dh in R.GELU_DH}
    return dict(u=u, ud=ud, n=n, y=y, dy=dy, fwd=fwd, bwd=bwd)


def test_gelu_every_operand(exhaustive):
    e = exhaustive
    got = e['fwd'].cpu()
    assert torch.isfinite(got).all()
    assert _note('gelu_bf16', 'all %d operands' % e['n'], R.worst(got.double() - e['y'], R.gelu_bound(e['y'], e['u']))) <= 1.0
    zero = e['u'].double() == 0
    assert zero.sum().item() == 2 + e['u'].numel() - e['n']
    assert torch.equal(_bits(got)[zero], _bits(e['u'])[zero]), 'gelu(+-0) is not +-0'


def test_gelu_backward_every_operand(exhaustive):
    e = exhaustive
    for dh in R.GELU_DH:
        got = e['bwd'][dh].cpu()
        assert torch.isfinite(got).all()
        ratio = R.worst(got.double() - dh * e['dy'], R.gelu_grad_bound(e['dy'], e['u'], dh))
        assert _note('gelu_bwd_bf16', 'all %d operands, dh %g' % (e['n'], dh), ratio) <= 1.0


@pytest.mark.parametrize('n', [8, 16, 8 * 257])
def test_gelu_ragged_sizes(exhaustive, n):
    """n operands drawn evenly, with wrap-around, from the 1536 patterns with 1/8 <= |u| < 8, where GELU is neither u nor 0; the
    sentinel behind n survives"""
    e = exhaustive
    band = ((e['u'].double().abs() >= 0.125) & (e['u'].double().abs() < 8)).nonzero().view(-1)
    assert band.numel() == 1536
    pick = band[torch.arange(n) * 191 % 1536]
    u = e['u'][pick]
    y, dy = e['y'][pick], e['dy'][pick]
    ud = u.cuda()
    got = _gelu(ud).cpu()
    assert _note('gelu_bf16', 'n = %d' % n, R.worst(got.double() - y, R.gelu_bound(y, u))) <= 1.0
    assert torch.equal(_bits(got), _bits(e['fwd'].cpu()[pick]))
    dh = R.GELU_DH[1]
    got = _gelu(ud, torch.full_like(ud, dh)).cpu()
    assert _note('gelu_bwd_bf16', 'n = %d' % n, R.worst(got.double() - dh * dy, R.gelu_grad_bound(dy, u, dh))) <= 1.0
    assert torch.equal(_bits(got), _bits(e['bwd'][dh].cpu()[pick]))


@pytest.mark.parametrize('items', [R.GRID_DEFAULT_ITEMS + 3, R.GELU_GRID_ITEMS + 3], ids=['default_cap', 'second_trip'])
def test_gelu_past_one_grid_trip(exhaustive, items):
    """the operand set tiled to 8 * items elements: the kernel is point-wise, so every element equals the exhaustive case's output
    for the same pattern wherever it sits.  R.GELU_GRID_ITEMS + 3 vectors are three more than k_gelu's grid covers in one trip"""
    e = exhaustive
    n = 8 * items
    m = e['u'].numel()
    reps = (n + m - 1) // m
    ud = e['ud'].repeat(reps)[:n].contiguous()
    assert torch.equal(_bits(_gelu(ud)), _bits(e['fwd'].repeat(reps)[:n]))
    dh = R.GELU_DH[1]
    assert torch.equal(_bits(_gelu(ud, torch.full_like(ud, dh))), _bits(e['bwd'][dh].repeat(reps)[:n]))
