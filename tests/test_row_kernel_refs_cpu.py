"""tests/_row_kernels_ref.py pinned without a GPU: every fp32 mirror meets its bound against the fp64 reference at every shape
tests/test_row_kernels_gpu.py runs (so no GPU test asks for more than fp32 can give), each listed wrong variant of a mirror exceeds
the bound on the same inputs (so the inputs and bounds can tell it apart), the generated inputs have the properties the GPU tests
rely on, and the host entries refuse what their headers forbid before any launch.

Worst |err| / bound of the mirrors (torch's CPU fp32; printed by the tests):
  LayerNorm forward   bf16 0.4935   pair 0.1295        LayerNorm backward   bf16 0.4925   pair 0.4370
  soft-max forward    bf16 0.4765   pair 0.1840        soft-max backward    bf16 0.4895   pair 0.2248
  GELU 0.4876         GELU' 0.4967
Three tests show why the bounds carry a term each that their first statement did not have (tests/_row_kernels_ref.py): without the
mean term the pair LayerNorm forward mirror is at 2.7 on row (a); without the dot term the soft-max backward mirror is at 128
(bf16) and 3e4 (pair) on rows that one probability dominates; and with two roundings of the dot instead of the count of them, a
plain fp32 dot taken in the pair kernel's lane order is at 1.135."""
import pytest
import torch

import _row_kernels_ref as R

PRECS = ('bf16', 'pair')
LN_IDS = ['%dx%d' % s for s in R.LN_SHAPES]
PLANTED = [s for s in R.LN_SHAPES if s[0] >= 6]
PLANTED_IDS = ['%dx%d' % s for s in PLANTED]
_worst = {}


def _note(name, ratio):
    _worst[name] = max(_worst.get(name, 0.0), ratio)
    print('%s: worst |err| / bound = %.4f (so far %.4f)' % (name, ratio, _worst[name]))
    return ratio


def _ln_fwd(c, prec, variant=None):
    """-> the worst |err| / bound of every row"""
    ref = R.ln_fwd_ref(c['x'], c['gamma'], c['beta'])
    bound, _ = R.ln_fwd_bound(c['x'], c['gamma'], c['beta'], prec)
    return R.worst_per_row(R.ln_fwd_mirror(c['x'], c['gamma'], c['beta'], prec, variant=variant) - ref, bound)


def _ln_bwd(c, prec, res, variant=None):
    ref = R.ln_bwd_ref(c['x'], c['dy'], c['gamma'], res)
    bound = R.ln_bwd_bound(c['x'], c['dy'], c['gamma'], res, prec)
    return R.worst_per_row(R.ln_bwd_mirror(c['x'], c['dy'], c['gamma'], res, prec, variant=variant) - ref, bound)


# ------------------------------------------------------------------ the mirrors meet the bounds
@pytest.mark.parametrize('shape', R.LN_SHAPES, ids=LN_IDS)
@pytest.mark.parametrize('prec', PRECS)
def test_layernorm_mirrors_meet_the_bounds(prec, shape):
    c = R.ln_case(*shape, prec)
    assert _note('layernorm forward mirror ' + prec, max(_ln_fwd(c, prec))) <= 1.0
    for res in (c['res'], None):
        assert _note('layernorm backward mirror ' + prec, max(_ln_bwd(c, prec, res))) <= 1.0


def test_layernorm_forward_bound_needs_the_mean_term():
    """as a pair, row (a) keeps its spread: the fp32 mean's rounding, times rstd = 20, exceeds the bound's first two terms"""
    over = 0.0
    for shape in PLANTED:
        c = R.ln_case(*shape, 'pair')
        ref = R.ln_fwd_ref(c['x'], c['gamma'], c['beta'])
        _, two = R.ln_fwd_bound(c['x'], c['gamma'], c['beta'], 'pair')
        over = max(over, R.worst_per_row(R.ln_fwd_mirror(c['x'], c['gamma'], c['beta'], 'pair') - ref, two)[R.ROW_A])
    print('pair layernorm forward mirror, row (a), against the first two terms alone: %.3f' % over)
    assert over > 1.0


@pytest.mark.parametrize('prec', PRECS)
def test_softmax_mirrors_meet_the_bounds(prec):
    for shape, rows in R.sm_cases(prec):
        for scale in R.SM_SCALES:
            c, n = R.sm_case(prec, shape, rows, scale), shape[0]
            ref = R.sm_fwd_ref(c['s'], n, scale)
            got = R.sm_fwd_mirror(c['s'], n, scale, prec)
            assert torch.isfinite(got).all()                  # the NaN slack stays out
            assert _note('soft-max forward mirror ' + prec, R.worst(got - ref, R.sm_fwd_bound(ref, prec))) <= 1.0, (shape, scale)
            bound = R.sm_bwd_bound(c['p'], c['dp'], n, scale, prec)
            for order in (None, 'lanes'):
                got = R.sm_bwd_mirror(c['p'], c['dp'], n, scale, prec, order=order)
                name = 'soft-max backward mirror %s%s' % (prec, ', the dot in lane order' if order else '')
                assert _note(name, R.worst(got - R.sm_bwd_ref(c['p'], c['dp'], n, scale), bound)) <= 1.0, (shape, scale)


@pytest.mark.parametrize('prec', PRECS)
def test_softmax_backward_bound_needs_the_dot_term(prec):
    """the planted row with its maximum in column 0, at scale 1: P[0] = 1 - delta, every value of the row is of the size of delta"""
    shape, scale = (197, 200, 224), 1.0
    c = R.sm_case(prec, shape, 6, scale)
    two = R.sm_bwd_bound(c['p'], c['dp'], shape[0], scale, prec, dot_roundings=0)
    err = R.sm_bwd_mirror(c['p'], c['dp'], shape[0], scale, prec) - R.sm_bwd_ref(c['p'], c['dp'], shape[0], scale)
    over = R.worst_per_row(err, two)[R.SM_MAX_FIRST]
    print('%s soft-max backward mirror, maximum-first row, against the first two terms alone: %.1f' % (prec, over))
    assert over > 1.0


def test_softmax_backward_dot_term_needs_the_rounding_count():
    """a plain fp32 dot in the pair kernel's own order (four columns per lane, fused multiply-adds, then across the lanes) is off by
    more than two roundings of the dot: n_valid = 5, scale 1, a row whose third probability is 0.99998"""
    shape, scale = (5, 8, 8), 1.0
    c = R.sm_case('pair', shape, 6, scale)
    bound = R.sm_bwd_bound(c['p'], c['dp'], shape[0], scale, 'pair')
    two_roundings = R.sm_bwd_bound(c['p'], c['dp'], shape[0], scale, 'pair', dot_roundings=2)
    err = R.sm_bwd_mirror(c['p'], c['dp'], shape[0], scale, 'pair', order='lanes') - R.sm_bwd_ref(c['p'], c['dp'], shape[0], scale)
    over, ok = R.worst(err, two_roundings), R.worst(err, bound)
    print('pair soft-max backward, lane-order dot, against two roundings of the dot: %.4f; against the count: %.4f' % (over, ok))
    assert over > 1.0 and ok <= 1.0


def test_softmax_backward_reference_is_autograd_of_the_softmax():
    """on probabilities that ARE the fp64 soft-max of the scores, the derivative applied to P equals autograd through the scores"""
    shape, scale = (197, 200, 224), 0.125
    c = R.sm_case('pair', shape, 6, scale)
    p = R.sm_fwd_ref(c['s'], shape[0], scale)
    a, b = R.sm_bwd_ref(p, c['dp'], shape[0], scale), R.sm_bwd_ref_from_scores(c['s'], c['dp'], shape[0], scale)
    assert (a - b).abs().max().item() <= 1e-15 * b.abs().max().item()


def test_gelu_mirrors_meet_the_bounds():
    u, _ = R.gelu_operands()
    y, dy = R.gelu_ref(u)
    got = R.gelu_mirror(u)
    assert torch.isfinite(got).all()
    assert _note('GELU mirror', R.worst(got - y, R.gelu_bound(y, u))) <= 1.0
    for dh in R.GELU_DH:
        got = R.gelu_grad_mirror(u, dh)
        assert torch.isfinite(got).all()
        assert _note("GELU' mirror", R.worst(got - dh * dy, R.gelu_grad_bound(dy, u, dh))) <= 1.0


# ------------------------------------------------------------------ the wrong variants exceed them
@pytest.mark.parametrize('shape', PLANTED, ids=PLANTED_IDS)
@pytest.mark.parametrize('prec', PRECS)
def test_layernorm_wrong_variants_exceed_the_bound(prec, shape):
    rows, dim = shape
    c = R.ln_case(rows, dim, prec)
    assert max(_ln_fwd(c, prec, 'unbiased')) > 1.0 and max(_ln_bwd(c, prec, c['res'], 'unbiased')) > 1.0
    assert _ln_fwd(c, prec, 'skip_last_vector')[R.ROW_C] > 1.0 and _ln_bwd(c, prec, None, 'skip_last_vector')[R.ROW_C] > 1.0
    assert _ln_fwd(c, prec, 'eps_outside')[R.ROW_D] > 1.0 and _ln_bwd(c, prec, c['res'], 'eps_outside')[R.ROW_D] > 1.0
    if dim in R.SLOT1_DIMS:
        assert _ln_fwd(c, prec, 'skip_slot1')[0] > 1.0 and _ln_bwd(c, prec, c['res'], 'skip_slot1')[0] > 1.0
    assert max(_ln_bwd(c, prec, c['res'], 'no_xhat_term')) > 1.0 and max(_ln_bwd(c, prec, None, 'no_xhat_term')) > 1.0


@pytest.mark.parametrize('shape', PLANTED, ids=PLANTED_IDS)
def test_layernorm_one_pass_variance_exceeds_the_bound_on_row_a(shape):
    """pair storage: bf16's step at 100 is 0.5, so in bf16 row (a) = 100 + 0.05 randn is the constant 100, whose one-pass variance
    is exactly 0 as well; the pair kernels see the spread, and share the bf16 kernels' statistics code line for line"""
    c = R.ln_case(*shape, 'pair')
    assert c['x'][R.ROW_A].std().item() > 0.02
    assert _ln_fwd(c, 'pair', 'one_pass')[R.ROW_A] > 1.0 and _ln_bwd(c, 'pair', c['res'], 'one_pass')[R.ROW_A] > 1.0
    b = R.ln_case(*shape, 'bf16')['x'][R.ROW_A]
    assert (b - 100).abs().max().item() <= 0.5


def _finite_slack(prec, shape, rows, scale):
    return R.sm_case(prec, shape, rows, scale, slack=(32.0, 1.0))


@pytest.mark.parametrize('prec', PRECS)
def test_softmax_wrong_variants_exceed_the_bound(prec):
    """with FINITE slack, at the shapes that have slack columns (a NaN would make these checks trivial): 1.0 in P and dP, and a score
    of 32 = four standard deviations, because one more score of ordinary size among a thousand moves a bf16 probability by less
    than its last place"""
    tried = [0, 0]
    for shape, rows in R.sm_cases(prec):
        n, ld_in, ld_out = shape
        for scale in R.SM_SCALES:
            c = _finite_slack(prec, shape, rows, scale)
            if ld_in > n:
                ref = R.sm_fwd_ref(c['s'], n, scale)
                assert R.worst(R.sm_fwd_mirror(c['s'], n, scale, prec, 'off_by_one') - ref, R.sm_fwd_bound(ref, prec)) > 1.0, (shape, scale)
                tried[0] += 1
            if min(ld_in, ld_out) > n:
                bound = R.sm_bwd_bound(c['p'], c['dp'], n, scale, prec)
                err = R.sm_bwd_mirror(c['p'], c['dp'], n, scale, prec, 'dot_over_ld') - R.sm_bwd_ref(c['p'], c['dp'], n, scale)
                assert R.worst(err, bound) > 1.0, (shape, scale)
                tried[1] += 1
    assert min(tried) >= 8


def test_gelu_wrong_variants_exceed_the_bound():
    u, _ = R.gelu_operands()
    y, dy = R.gelu_ref(u)
    tail = (u.double() >= -5) & (u.double() <= -3)
    assert R.worst((R.gelu_mirror(u, 'tanh') - y)[tail], R.gelu_bound(y, u)[tail]) > 1.0           # the negative tail tells them apart
    for dh in R.GELU_DH:
        assert R.worst(R.gelu_grad_mirror(u, dh, 'no_v_phi') - dh * dy, R.gelu_grad_bound(dy, u, dh)) > 1.0


# ------------------------------------------------------------------ the inputs are what the GPU tests rely on
@pytest.mark.parametrize('prec', PRECS)
def test_planted_rows(prec):
    for rows, dim in PLANTED:
        c = R.ln_case(rows, dim, prec)
        x = c['x']
        assert torch.equal(x[R.ROW_B], torch.full((dim,), 3.25))                    # constant after rounding
        assert x[R.ROW_C, dim - 1].item() == 50 and (x[R.ROW_C, :dim - 1] == 0).all()
        var_d = x[R.ROW_D].double().var(unbiased=False).item()
        assert 0.2 * R.EPS < var_d < 5 * R.EPS
        assert abs(x[R.ROW_A].mean().item() - 100) < 0.1
        for k in ('x', 'dy', 'res'):
            assert torch.equal(c[k][rows - 1], c[k][0])
            pl = R.planes(c[k], prec)
            assert torch.equal(R.value64(pl), c[k].double())                          # the planes hold exactly these values
            if prec == 'pair':
                assert torch.equal(R.split(c[k]), torch.stack(pl))                    # stable under re-splitting
    assert not R.ln_case(1, 768, prec)['planted']


@pytest.mark.parametrize('prec', PRECS)
def test_score_rows(prec):
    for shape, rows in R.sm_cases(prec):
        n, ld_in, ld_out = shape
        for scale in R.SM_SCALES:
            c = R.sm_case(prec, shape, rows, scale)
            s, p, dp = c['s'], c['p'], c['dp']
            assert s.shape == (rows, ld_in) and p.shape == (rows, ld_out) and dp.shape == (rows, ld_in)
            for t in (s, p, dp):
                assert torch.isnan(t[:, n:]).all() and torch.isfinite(t[:, :n]).all()
                if prec == 'bf16':
                    assert torch.equal(t[:, :n], t[:, :n].to(torch.bfloat16).float())
            if prec == 'pair':
                assert torch.equal(R.canonical(p[:, :n]), p[:, :n])                   # stable under re-splitting
            assert (s[R.SM_EQUAL, :n] == s[R.SM_EQUAL, 0]).all()
            assert s[R.SM_ONE_HOT, n - 1].item() == 300 and (s[R.SM_ONE_HOT, :n - 1] == -300).all()
            assert s[R.SM_MAX_FIRST, :n].argmax().item() == 0
            assert (p[:, :n].double().sum(-1) - 1).abs().max().item() <= ld_out * 2.0 ** -8


def test_gelu_operand_set():
    bits = R.gelu_patterns()
    assert bits.numel() == 58114 and bits.unique().numel() == 58114
    u, n = R.gelu_operands()
    assert n == 58114 and u.numel() == 58120 and u.numel() % 8 == 0 and (u[n:].view(torch.int16) == 0).all()
    v = u[:n].double()
    assert torch.isfinite(v).all()
    mag = v.abs()[v != 0]
    assert mag.min().item() == 2.0 ** -100 and mag.max().item() == 2.0 ** 127 * (1 - 2.0 ** -8)
    assert (bits == -32768).sum().item() == 1 and (bits == 0).sum().item() == 1                 # -0.0 and +0.0
    assert (v > 14).any() and (v < -14).any() and ((v >= -5) & (v <= -3)).sum().item() == 97
    assert R.GRID_DEFAULT_ITEMS == 2048 * 256 and R.GELU_GRID_ITEMS == 2 * R.GRID_DEFAULT_ITEMS


# ------------------------------------------------------------------ host refusals: nothing is launched
def test_row_entries_refuse_what_their_headers_forbid_without_gpu():
    from robustart_amd import _lib
    lib = _lib.load()
    p, e = 4096, 1e-6                                       # never dereferenced

    def ln(prec, dim, ld_in, ld_out):
        if prec == 'bf16':
            return lib.rart_layernorm_bf16(p, p, p, 2 * p, 4, dim, ld_in, ld_out, e, None)
        return lib.rart_layernorm_pair(p, p, p, p, 2 * p, 2 * p, 4, dim, ld_in, ld_out, e, None)

    def ln_bwd(prec, dim, strides, res=True):
        r = p if res else None
        if prec == 'bf16':
            return lib.rart_layernorm_bwd_bf16(p, p, p, r, 2 * p, 4, dim, *strides, e, None)
        return lib.rart_layernorm_bwd_pair(p, p, p, p, p, r, r, 2 * p, 2 * p, 4, dim, *strides, e, None)

    for prec in PRECS:
        for dim in (1032, 12):
            assert ln(prec, dim, 2048, 2048) != 0 and ln_bwd(prec, dim, (2048,) * 4) != 0, (prec, dim)
        for k in range(2):
            assert ln(prec, 8, *[12 if j == k else 16 for j in range(2)]) != 0, (prec, k)
        for k in range(4):
            assert ln_bwd(prec, 8, [12 if j == k else 16 for j in range(4)]) != 0, (prec, k)
        assert ln(prec, 0, 16, 16) != 0 and ln_bwd(prec, 8, (16, 16, 12, 16), res=False) != 0

    def sm(prec, n, ld_in, ld_out):
        if prec == 'bf16':
            return lib.rart_softmax_rows_bf16(p, 2 * p, 4, n, ld_in, ld_out, 0.125, None)
        return lib.rart_softmax_rows_pair(p, 2 * p, 2 * p, 4, n, ld_in, ld_out, 0.125, None)

    def sm_bwd(prec, n, ld_p, ld_dp, ld_out):
        if prec == 'bf16':
            return lib.rart_softmax_bwd_rows_bf16(p, p, 2 * p, 4, n, ld_p, ld_dp, ld_out, 0.125, None)
        return lib.rart_softmax_bwd_rows_pair(p, p, p, 2 * p, 2 * p, 4, n, ld_p, ld_dp, ld_out, 0.125, None)

    for prec, big, small, ok in (('bf16', 1032, 12, 16), ('pair', 260, 6, 8)):
        for bad in (big, small):
            for k in range(2):
                assert sm(prec, 4, *[bad if j == k else ok for j in range(2)]) != 0, (prec, bad, k)
            for k in range(3):
                assert sm_bwd(prec, 4, *[bad if j == k else ok for j in range(3)]) != 0, (prec, bad, k)
        for k in range(2):                                  # n_valid greater than a leading dimension
            assert sm(prec, 2 * ok, *[ok if j == k else 2 * ok for j in range(2)]) != 0, (prec, k)
        for k in range(3):
            assert sm_bwd(prec, 2 * ok, *[ok if j == k else 2 * ok for j in range(3)]) != 0, (prec, k)
    for n in (12, 0):
        assert lib.rart_gelu_bf16(p, 2 * p, n, None) != 0 and lib.rart_gelu_bwd_bf16(p, p, 2 * p, n, None) != 0, n
