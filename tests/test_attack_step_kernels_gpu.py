"""Kernel-level tests of csrc/attack_steps.hip: every step kernel against an fp64 restatement of the same operation
(tests/_attack_steps_ref.py, itself checked on the CPU by tests/test_attack_step_refs_cpu.py) at the row lengths where the chunking
can go wrong (RCH = 32 chunks per row, 256- and 512-thread workgroups, float4 lanes), with rows of very different norms, a
zero-gradient row, guard bands around every float operand, and the native draws pinned word for word to the host generator.

For every in-place kernel: the guard bands and the read-only operands are unchanged, a second call gives identical bits, and row r
computed inside the batch equals row r computed alone, bit for bit (the batch-splitting invariance AutoAttack relies on)."""
import ctypes

import numpy as np
import pytest
import torch

import _attack_steps_ref as R
from oracle import attacks_ref as A

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x7FC5A5A5                     # a quiet NaN: a reduction that reads a guard band is poisoned, a write to one is seen
SHAPES = pytest.mark.parametrize('batch,nps', R.SHAPES)


def _lib():
    from robustart_amd import _lib as L
    return L


class Arena:
    """float operands inside larger allocations: GUARD sentinel words on both sides of each"""

    def __init__(self):
        self.items = []

    def _put(self, shape, src, readonly, offset):
        n = int(np.prod(shape))
        buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, dtype=torch.int32, device='cuda')
        view = buf[GUARD + offset:GUARD + offset + n].view(torch.float32).view(*shape)
        if src is not None:
            view.copy_(src)
        self.items.append((buf, offset, n, view, src.clone() if readonly else None))
        return view

    def ro(self, t, offset=0):
        return self._put(tuple(t.shape), t, True, offset)

    def rw(self, t, offset=0):
        return self._put(tuple(t.shape), t, False, offset)

    def out(self, *shape):
        return self._put(shape, None, False, 0)            # starts as sentinels: an element the kernel skips stays NaN

    def done(self, **outs):
        torch.cuda.synchronize()
        res = {k: v.cpu() for k, v in outs.items()}
        for buf, offset, n, view, orig in self.items:
            b = buf.cpu()
            assert (b[:GUARD + offset] == SENTINEL).all() and (b[GUARD + offset + n:] == SENTINEL).all(), 'guard band overwritten'
            if orig is not None:
                assert R.same_bits(view.cpu(), orig), 'read-only operand changed'
        return res


def _check_invariances(run, c, got):
    """second call: same bits; row r alone == row r in the batch; the batch without the zero-gradient row == the other rows"""
    batch = next(iter(c.values())).shape[0]
    again = run(c)
    for k in got:
        assert R.same_bits(again[k], got[k]), 'second call differs in ' + k
    if batch == 1:
        return
    for r in R.rows_to_check(batch):
        alone = run(R.rows_of(c, [r]))
        for k in got:
            assert R.same_bits(alone[k][0], got[k][r]), 'row %d alone differs from row %d in the batch (%s)' % (r, r, k)
    if batch >= 3:
        keep = [b for b in range(batch) if b != R.DEAD_ROW]
        sub = run(R.rows_of(c, keep))
        for k in got:
            assert R.same_bits(sub[k], got[k][keep]), 'rows change when the zero-gradient row leaves the batch (%s)' % k


def _report(name, batch, nps, err, bound, extra=''):
    print('attack-step error: %-22s %4d x %-6d %.3e (bound %.3e)%s' % (name, batch, nps, err, bound, extra))


def _maxerr(got, want64):
    return (got.double() - want64).abs().max().item()


def _in_box(t):
    return bool(torch.isfinite(t).all()) and t.min().item() >= 0.0 and t.max().item() <= 1.0


# ---- PGD-Linf: float4 body, scalar tail, the unaligned branch ------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3, 5, 1029, R.IMAGENET_ROW * 7])
@pytest.mark.parametrize('misaligned', ['none', 'x', 'g', 'all'])
def test_pgd_step_linf_is_bit_exact_on_aligned_and_offset_views(n, misaligned):
    """Bit-exact against A.pgd_linf_step in fp32 on 16-byte aligned buffers (float4 body + tail from 4 * (n / 4)) and on views offset by
    one float -- x only, g only, all three -- where al == false and every element goes through k_pgd_linf_tail."""
    from robustart_amd.noise import adv
    d = R.inputs(1, n)
    x, g, x0 = R.start_point(d, 'Linf', R.EPS_LINF)[0], d['g'][0], d['x0'][0]
    alpha = R.f32(R.EPS_LINF * 3 / 40)
    want = A.pgd_linf_step(x, g, x0, R.EPS_LINF, alpha)
    ar = Arena()
    xg = ar.rw(x, 1 if misaligned in ('x', 'all') else 0)
    gg = ar.ro(g, 1 if misaligned in ('g', 'all') else 0)
    x0g = ar.ro(x0, 1 if misaligned == 'all' else 0)
    assert (xg.data_ptr() % 16 == 0) == (misaligned not in ('x', 'all'))
    adv.pgd_step_linf_(xg, gg, x0g, R.EPS_LINF, alpha)
    got = ar.done(x=xg)['x']
    assert torch.equal(got, want), (got - want).abs().max()
    assert _in_box(got) and (got - x0).abs().max() <= R.EPS_LINF + 1e-7


def test_pgd_step_linf_of_no_elements_returns_ok():
    L = _lib()
    d = R.inputs(1, 5)
    ar = Arena()
    x, g, x0 = ar.ro(d['u'][0]), ar.ro(d['g'][0]), ar.ro(d['x0'][0])
    assert L.load().rart_pgd_step_linf(L.ptr(x), L.ptr(g), L.ptr(x0), 0, R.EPS_LINF, 0.01, L.stream_ptr()) == 0
    ar.done()


# ---- row-reduced steps -----------------------------------------------------------------------------------------------------------------
def _run_pgd_l2(c):
    from robustart_amd.noise import adv
    ar = Arena()
    x, g, x0 = ar.rw(c['x']), ar.ro(c['g']), ar.ro(c['x0'])
    adv.pgd_step_l2_(x, g, x0, R.EPS_L2, R.PGD_L2_ALPHA)
    return ar.done(x=x)


@SHAPES
def test_pgd_step_l2_vs_fp64(batch, nps):
    c = R.step_case('pgd_l2', batch, nps)
    got = _run_pgd_l2(c)
    x64, g64, x064 = R.dbl(c['x'], c['g'], c['x0'])
    want = R.pgd_l2_step(x64, g64, x064, R.EPS_L2, R.PGD_L2_ALPHA)
    err = _maxerr(got['x'], want)
    _report('rart_pgd_step_l2', batch, nps, err, 1e-6)
    assert err <= 1e-6
    assert _in_box(got['x']) and ((got['x'].double() - x064).pow(2).sum(1).sqrt() <= R.EPS_L2 + 1e-5).all()
    if batch >= 3:                                       # zero gradient: the step is the projection of its input
        d = (x64 - x064)[R.DEAD_ROW]
        proj = torch.clamp(x064[R.DEAD_ROW] + d * min(R.EPS_L2 / max(d.norm().item(), 1e-12), 1.0), 0, 1)
        assert _maxerr(got['x'][R.DEAD_ROW], proj) <= 1e-6
    _check_invariances(_run_pgd_l2, c, got)


def _run_pgd_l1(c):
    from robustart_amd.noise import adv
    eps = R.eps_l1(c['x'].shape[1])
    ar = Arena()
    x, g, x0 = ar.rw(c['x']), ar.ro(c['g']), ar.ro(c['x0'])
    adv.pgd_step_l1_(x, g, x0, eps, eps / 8)
    return ar.done(x=x)


@SHAPES
def test_pgd_step_l1_vs_fp64(batch, nps):
    """Bound = 8 x (the fp32 torch restatement's error against fp64 on the same inputs) + one ulp at 1.0 (R.l1_bound): the kernel sums
    |g| and |delta| in another, equally valid order."""
    c = R.step_case('pgd_l1', batch, nps)
    eps = R.eps_l1(nps)
    got = _run_pgd_l1(c)
    x64, g64, x064 = R.dbl(c['x'], c['g'], c['x0'])
    want = R.pgd_l1_step(x64, g64, x064, eps, eps / 8)
    err32 = _maxerr(R.pgd_l1_step(c['x'], c['g'], c['x0'], eps, eps / 8), want)
    err, bound = _maxerr(got['x'], want), R.l1_bound(err32)
    _report('rart_pgd_step_l1', batch, nps, err, bound, ' fp32 restatement %.3e' % err32)
    assert err <= bound
    assert _in_box(got['x']) and ((got['x'].double() - x064).abs().sum(1) <= eps * (1 + 1e-5)).all()
    if batch >= 3:
        x1 = torch.clamp(x64[R.DEAD_ROW], 0, 1)
        d = x1 - x064[R.DEAD_ROW]
        proj = d * min(1.0, eps / (d.abs().sum().item() + R.ART_TOL)) + x064[R.DEAD_ROW]
        assert _maxerr(got['x'][R.DEAD_ROW], proj) <= bound
    _check_invariances(_run_pgd_l1, c, got)


def _run_mim(c):
    from robustart_amd.noise import adv
    ar = Arena()
    x, m, g, x0 = ar.rw(c['x']), ar.rw(c['m']), ar.ro(c['g']), ar.ro(c['x0'])
    adv.mim_step_(x, m, g, x0, R.EPS_LINF, R.MIM_STEP, R.MIM_DECAY)
    return ar.done(x=x, m=m)


@SHAPES
def test_mim_step_vs_fp64(batch, nps):
    """x within 1e-6 and the momentum within relative 1e-5 of fp64.  x steps by step * sign(m): where the fp64 momentum is below
    MIM_M_EXCLUDE the fp32 momentum may have the other sign, those elements (at most MIM_EXCLUDE_CAP of the tensor, a cap the CPU
    module proves for the reference on every input used here) are only required to be the projection of a point within step_size of
    the input x: P(x - step) <= x_new <= P(x + step), P being monotone.
    The zero-gradient row: the reference divides by the zero mean |g| and returns NaN everywhere.  The kernel's momentum of that row
    is NaN too (0 / 0), sign(NaN) is taken as 0, so x becomes the projection of its input: finite and feasible.  m is not asserted."""
    c = R.step_case('mim', batch, nps)
    got = _run_mim(c)
    live = [b for b in range(batch) if not (batch >= 3 and b == R.DEAD_ROW)]
    x64, m64, g64, x064 = (c[k][live].double() for k in ('x', 'm', 'g', 'x0'))
    wx, wm = R.mim_step(x64, g64, m64, x064, R.EPS_LINF, R.MIM_STEP, R.MIM_DECAY)
    gx, gm = got['x'][live].double(), got['m'][live].double()
    assert ((gm - wm).abs() <= 1e-5 + 1e-5 * wm.abs()).all(), ((gm - wm).abs() / (1 + wm.abs())).max()
    skip = wm.abs() < R.MIM_M_EXCLUDE
    assert skip.sum().item() <= R.MIM_EXCLUDE_CAP * wm.numel()
    err = (gx - wx).abs()[~skip].max().item() if (~skip).any() else 0.0
    _report('rart_mim_step x', batch, nps, err, 1e-6, ' momentum rel %.3e, %d skipped' % (((gm - wm).abs() / (1 + wm.abs())).max().item(),
                                                                                       int(skip.sum())))
    assert err <= 1e-6
    lo = R.linf_project(x64 - R.MIM_STEP, x064, R.EPS_LINF) - 1e-6
    hi = R.linf_project(x64 + R.MIM_STEP, x064, R.EPS_LINF) + 1e-6
    assert ((gx >= lo) & (gx <= hi))[skip].all()
    assert _in_box(got['x']) and ((got['x'] - c['x0']).abs() <= R.EPS_LINF + 1e-7).all()          # the dead row included
    _check_invariances(_run_mim, c, got)


def _run_apgd(norm, a):
    def run(c):
        from robustart_amd.noise import adv
        ar = Arena()
        xa, xold, g, x0, step = ar.rw(c['xa']), ar.rw(c['xold']), ar.ro(c['g']), ar.ro(c['x0']), ar.ro(c['step'])
        adv.apgd_step_(xa, xold, g, x0, step, norm, R.EPS_LINF if norm == 'Linf' else R.EPS_L2, a)
        return ar.done(xa=xa, xold=xold)
    return run


@pytest.mark.parametrize('a', [1.0, 0.75])
@pytest.mark.parametrize('norm', ['Linf', 'L2'])
@SHAPES
def test_apgd_step_vs_fp64(batch, nps, norm, a):
    """L2: within 2e-6 of fp64.  Linf: bit-exact (tolerance 0) against the same expression in fp32, as tests/test_attacks_gpu.py holds
    it -- no fp32 result can be at distance 0 from fp64 (the fp32 oracle itself is up to 9e-8 away, CPU module) -- and within 4 ulp at
    1.0 of fp64: the step is elementwise and continuous in everything but sign(grad), which is exact, and rounds 5 values below 2.
    step differs per row by factors of 4.  The zero-gradient row is part of the comparison (its reference is the projection of the
    momentum-extrapolated input, no division by zero: g / (0 + 1e-12) = 0)."""
    eps = R.EPS_LINF if norm == 'Linf' else R.EPS_L2
    c = R.step_case('apgd_' + norm, batch, nps)
    run = _run_apgd(norm, a)
    got = run(c)
    want = R.apgd_step(*R.dbl(c['xa'], c['xold'], c['g'], c['x0']), eps, c['step'], a, norm)
    err, tol = _maxerr(got['xa'], want), (4 * R.ULP1 if norm == 'Linf' else 2e-6)
    _report('rart_apgd_step %s a=%g' % (norm, a), batch, nps, err, tol)
    assert err <= tol
    if norm == 'Linf':
        assert torch.equal(got['xa'], R.apgd_step(c['xa'], c['xold'], c['g'], c['x0'], eps, c['step'], a, norm))
        assert ((got['xa'] - c['x0']).abs() <= eps + 1e-7).all()
    else:
        assert ((got['xa'].double() - c['x0'].double()).pow(2).sum(1).sqrt() <= eps + 1e-5).all()
    assert R.same_bits(got['xold'], c['xa']) and _in_box(got['xa'])
    _check_invariances(run, c, got)


def _run_apgd_init(norm):
    def run(c):
        L = _lib()
        from robustart_amd.noise import adv
        batch, nps = c['x0'].shape
        eps = {'Linf': R.EPS_LINF, 'L2': R.EPS_L2, 'L1': R.eps_l1(nps)}[norm]
        ar = Arena()
        x, x0, t = ar.out(batch, nps), ar.ro(c['x0']), ar.ro(c['t'])
        ws, nb = adv._ws(batch, 'cuda')
        L.check(L.load().rart_apgd_init(L.ptr(x), L.ptr(x0), batch, nps, {'Linf': 0, 'L2': 1, 'L1': 2}[norm], eps, 0, 0, None, L.ptr(t),
                                        L.ptr(ws), nb, L.stream_ptr()))
        return ar.done(x=x)
    return run


@pytest.mark.parametrize('norm', ['Linf', 'L2', 'L1'])
@SHAPES
def test_apgd_init_injected_vs_fp64(batch, nps, norm):
    d = R.inputs(batch, nps)
    c = dict(x0=d['x0'], t=d['t_uniform'] if norm == 'Linf' else d['t_normal'])
    eps = {'Linf': R.EPS_LINF, 'L2': R.EPS_L2, 'L1': R.eps_l1(nps)}[norm]
    run = _run_apgd_init(norm)
    got = run(c)
    err = _maxerr(got['x'], R.apgd_start(c['x0'].double(), c['t'].double(), norm, eps))
    _report('rart_apgd_init ' + norm, batch, nps, err, 1e-7)
    assert err <= 1e-7 and _in_box(got['x'])
    _check_invariances(run, c, got)


def _run_l1_start(c):
    L = _lib()
    from robustart_amd.noise import adv
    batch, nps = c['x0'].shape
    ar = Arena()
    x, x0, se, rad = ar.out(batch, nps), ar.ro(c['x0']), ar.ro(c['se']), ar.ro(c['radius'])
    ws, nb = adv._ws(batch, 'cuda')
    L.check(L.load().rart_random_start_l1(L.ptr(x), L.ptr(x0), batch, nps, R.eps_l1(nps), 0, 0, None, L.ptr(se), L.ptr(rad), L.ptr(ws), nb,
                                          L.stream_ptr()))
    return ar.done(x=x)


@SHAPES
def test_random_start_l1_injected_vs_fp64(batch, nps):
    """injected signed exponentials and radii; bound as for the PGD-L1 step (R.l1_bound)"""
    c = R.step_case('l1_start', batch, nps)
    got = _run_l1_start(c)
    want = R.l1_sphere_start(*R.dbl(c['x0'], c['se'], c['radius']))
    err32 = _maxerr(R.l1_sphere_start(c['x0'], c['se'], c['radius']), want)
    err, bound = _maxerr(got['x'], want), R.l1_bound(err32)
    _report('rart_random_start_l1', batch, nps, err, bound, ' fp32 restatement %.3e' % err32)
    assert err <= bound
    assert _in_box(got['x']) and ((got['x'].double() - c['x0'].double()).abs().sum(1) <= R.eps_l1(nps) * (1 + 1e-5)).all()
    _check_invariances(_run_l1_start, c, got)


# ---- random starts: injected form, and the native draws against the host mirror ---------------------------------------------------------
def _init_linf(x0, eps, clip, seed=0, sample_offset=0, rows=None, inj=None):
    L = _lib()
    batch, nps = x0.shape
    ar = Arena()
    x, x0g = ar.out(batch, nps), ar.ro(x0)
    injg = ar.ro(inj) if inj is not None else None
    rg = torch.tensor(rows, dtype=torch.int64, device='cuda') if rows is not None else None
    lo, hi = (0.0, 1.0) if clip else (1.0, 0.0)
    L.check(L.load().rart_attack_init_linf(L.ptr(x), L.ptr(x0g), batch, nps, eps, lo, hi, seed, sample_offset, L.ptr(rg), L.ptr(injg),
                                           L.stream_ptr()))
    return ar.done(x=x)['x']


@pytest.mark.parametrize('clip', [True, False])
@SHAPES
def test_attack_init_linf_injected_is_bit_exact(batch, nps, clip):
    d = R.inputs(batch, nps)
    u = d['t_uniform'] * torch.tensor(R.EPS_LINF)
    got = _init_linf(d['x0'], R.EPS_LINF, clip, inj=u)
    want = d['x0'] + u
    assert torch.equal(got, torch.clamp(want, 0.0, 1.0) if clip else want)
    assert R.same_bits(got, _init_linf(d['x0'], R.EPS_LINF, clip, inj=u))
    for r in R.rows_to_check(batch)[:3]:
        assert R.same_bits(_init_linf(d['x0'][r:r + 1], R.EPS_LINF, clip, inj=u[r:r + 1])[0], got[r])


@SHAPES
def test_attack_init_linf_native_draws_match_the_host_mirror(batch, nps):
    """element e of row b = x0 + eps * (2 u01(word) - 1), word = .x / .y of counter (e >> 1, stream 1) at sample sample_offset + b.
    Within 2^-23 of the mirror: a wrong counter, lane, stream or sample mapping is off by O(eps)."""
    if batch > 7:
        batch = 70                                                  # (rows beyond the 4100 case's point: the mirror costs host time)
    d = R.inputs(batch, nps)
    seed, off = (0x9E3779B9 << 32) | 12345, 17
    got = _init_linf(d['x0'], R.EPS_LINF, True, seed, off)
    want = R.native_init_linf(d['x0'], R.EPS_LINF, seed, R.row_samples(batch, off))
    err = _maxerr(got, want.double())
    _report('rart_attack_init_linf', batch, nps, err, R.ULP1, ' (native draws vs the host mirror)')
    assert err <= R.ULP1
    noclip = _init_linf(d['x0'], R.EPS_LINF, False, seed, off)
    assert _maxerr(noclip, R.native_init_linf(d['x0'], R.EPS_LINF, seed, R.row_samples(batch, off), clip=False).double()) <= R.ULP1


@pytest.mark.parametrize('nps', [33, 257])
def test_native_draws_are_keyed_by_the_global_sample_index(nps):
    """row_samples = [5, 2, 9] gives rows 5, 2, 9 of a contiguous call at offset 0; sample_offset = 100 gives rows 100.. of offset 0"""
    x0 = R.inputs(3, nps)['x0']
    big = x0[torch.arange(103) % 3]
    full = _init_linf(big, R.EPS_LINF, True, 7, 0)
    pick = [5, 2, 9]
    got = _init_linf(big[pick], R.EPS_LINF, True, 7, 0, rows=pick)
    assert R.same_bits(got, full[pick])
    assert R.same_bits(_init_linf(big[100:], R.EPS_LINF, True, 7, 100), full[100:])
    assert not torch.equal(full[0], full[3])                       # same x0 row, another sample: another draw


@pytest.mark.parametrize('batch,nps', [(1, 1), (3, 33), (7, 257), (3, 1029), (7, R.IMAGENET_ROW)])
def test_apgd_init_native_linf_matches_the_host_mirror(batch, nps):
    """x against the op-by-op mirror within 2^-23; with x0 = 0.5 and eps = 0.25 (x - x0 and the division by eps are exact) the
    implied t / max |t| against the mirror's within 2^-23 too."""
    L = _lib()
    from robustart_amd.noise import adv
    seed, rows = 99, [3 + 2 * b for b in range(batch)]
    for x0, eps in ((R.inputs(batch, nps)['x0'], R.EPS_LINF), (torch.full((batch, nps), 0.5), 0.25)):
        ar = Arena()
        x, x0g = ar.out(batch, nps), ar.ro(x0)
        ws, nb = adv._ws(batch, 'cuda')
        rg = torch.tensor(rows, dtype=torch.int64, device='cuda')
        L.check(L.load().rart_apgd_init(L.ptr(x), L.ptr(x0g), batch, nps, 0, eps, seed, 0, L.ptr(rg), None, L.ptr(ws), nb, L.stream_ptr()))
        got = ar.done(x=x)['x']
        want, tn = R.native_apgd_init_linf(x0, eps, seed, R.row_samples(batch, rows=rows))
        err = _maxerr(got, want.double())
        assert err <= R.ULP1 and _in_box(got)
        if eps == 0.25:
            implied = (got - 0.5) / 0.25
            ierr = _maxerr(implied, tn.double())
            _report('rart_apgd_init native', batch, nps, ierr, R.ULP1, ' (implied t / max|t| vs the host mirror; x %.3e)' % err)
            assert ierr <= R.ULP1 and implied.abs().max() <= 1.0


@pytest.mark.parametrize('batch,nps', [(3, 5), (3, 257), (7, 8191)])
def test_random_start_l1_native_matches_the_host_mirror(batch, nps):
    """signs exactly the mirror's (.y & 1 of counter e, stream 5); x within 1e-5 |delta| + 2^-23 of the mirror evaluated in fp64 from the
    same fp32 uniforms: logf and the fp32 sum of the exponentials are each good to a few ulp (1e-6 relative), a wrong counter, stream
    or sample mapping moves delta by its own size."""
    from robustart_amd.noise import adv
    x0 = 0.25 + 0.5 * R.inputs(batch, nps)['x0']                    # interior: nothing is clipped
    eps, seed, off = R.f32(0.002 * nps), 31, 40
    got = adv.random_start_l1(x0.cuda(), eps, seed=seed, sample_offset=off).cpu()
    se, rad = R.native_l1_start_draws(seed, R.row_samples(batch, off), nps, eps)
    delta = se * (rad / se.abs().sum(1)).view(-1, 1)
    assert torch.equal(torch.sign(got - x0).double()[delta.abs() > 1e-6], torch.sign(delta)[delta.abs() > 1e-6])
    assert ((got.double() - (x0.double() + delta)).abs() <= 1e-5 * delta.abs() + R.ULP1).all()
    assert ((got.double() - x0.double()).abs().sum(1) <= eps * (1 + 1e-5)).all()


# ---- Square, Linf ----------------------------------------------------------------------------------------------------------------------
def _square_init(x0, eps, seed=0, sample_offset=0, rows=None, inj=None):
    L = _lib()
    B, C, H, W = x0.shape
    ar = Arena()
    xb, x0g = ar.out(B, C, H, W), ar.ro(x0)
    injg = ar.ro(inj) if inj is not None else None
    rg = torch.tensor(rows, dtype=torch.int64, device='cuda') if rows is not None else None
    L.check(L.load().rart_square_init_linf(L.ptr(xb), L.ptr(x0g), B, C, H, W, eps, seed, sample_offset, L.ptr(rg), L.ptr(injg),
                                           L.stream_ptr()))
    return ar.done(xb=xb)['xb']


@pytest.mark.parametrize('shape', [(3, 3, 7, 5), (2, 3, 32, 32), (1, 1, 1, 1)])
def test_square_init_linf_signs_and_injected_form(shape):
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(5)
    x0 = 0.1 + 0.8 * torch.rand(shape, generator=gen)              # inside (eps, 1 - eps): the sign survives the clamp
    seed = 4242
    for off, rows in ((0, None), (11, None), (0, [9, 4, 6][:B])):
        got = _square_init(x0, R.EPS_LINF, seed, off, rows)
        sg = R.native_square_signs(seed, R.row_samples(B, off, rows), C, W)
        assert torch.equal(torch.sign(got - x0), sg.unsqueeze(2).expand(B, C, H, W))
        assert torch.equal(got, R.square_init_linf(x0, R.EPS_LINF, sg))
    x0e = R.inputs(B, C * H * W)['x0'].view(shape)                  # with exact 0.0 / 1.0 entries
    inj = torch.sign(torch.rand(B, C, W, generator=gen) - 0.5)
    assert torch.equal(_square_init(x0e, R.EPS_LINF, inj=inj), R.square_init_linf(x0e, R.EPS_LINF, inj))


def _square_propose(xb, x0, eps, vh, vw, s, signs):
    L = _lib()
    B, C, H, W = x0.shape
    ar = Arena()
    xn, xbg, x0g = ar.out(B, C, H, W), ar.ro(xb), ar.ro(x0)
    sg = (ctypes.c_float * C)(*[float(v) for v in signs])
    L.check(L.load().rart_square_propose_linf(L.ptr(xn), L.ptr(xbg), L.ptr(x0g), B, C, H, W, eps, vh, vw, s, sg, L.stream_ptr()))
    return ar.done(xn=xn)['xn']


@pytest.mark.parametrize('shape', [(3, 3, 7, 5), (2, 3, 32, 32)])
def test_square_propose_linf_is_bit_exact(shape):
    """windows at (0, 0), flush with the bottom-right corner, s = 1 and the largest s the image takes (s = H at 32 x 32; on the 7 x 5
    image s = W: a window of side H = 7 does not fit and is refused)"""
    B, C, H, W = shape
    x0 = R.inputs(B, C * H * W)['x0'].view(shape)
    signs0 = torch.sign(R.inputs(B, C * H * W)['t_uniform']).view(shape)[:, :, 0, :]
    xb = R.square_init_linf(x0, R.EPS_LINF, signs0)
    smax = min(H, W)
    windows = [(0, 0, 2), (H - 2, W - 2, 2), (0, 0, 1), (H - 1, W - 1, 1), (3, 2, 1), (0, 0, smax), (H - smax, W - smax, smax), (1, 1, 3)]
    for k, (vh, vw, s) in enumerate(windows):
        signs = [1.0 if (k >> c) & 1 else -1.0 for c in range(C)]
        got = _square_propose(xb, x0, R.EPS_LINF, vh, vw, s, signs)
        want = R.square_propose_linf(xb, x0, R.EPS_LINF, vh, vw, s, signs)
        assert torch.equal(got, want), (vh, vw, s)
        inside = torch.zeros(shape, dtype=torch.bool)
        inside[:, :, vh:vh + s, vw:vw + s] = True
        assert R.same_bits(got[~inside], xb[~inside]) and (got != xb).any()          # only the window moves, and it does move
    if H > W:
        with pytest.raises(_lib().RartError, match='window outside the image'):
            _square_propose(xb, x0, R.EPS_LINF, 0, 0, H, [1.0] * C)


# ---- expectation over transformation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 257, R.IMAGENET_ROW * 2])
def test_eot_accumulate_is_bit_exact(n):
    L = _lib()
    d = R.inputs(1, n)
    acc, g = d['g'][0] * 1e3, d['m'][0]
    ar = Arena()
    a, gg = ar.rw(acc), ar.ro(g)
    L.check(L.load().rart_eot_accumulate(L.ptr(a), L.ptr(gg), n, 0, 1.0, L.stream_ptr()))
    want = R.eot_accumulate(acc, g, 0, None)
    assert torch.equal(ar.done(a=a)['a'], want)
    for div in (3.0, 20.0):
        ar = Arena()
        a = ar.rw(want)
        L.check(L.load().rart_eot_accumulate(L.ptr(a), None, n, 1, div, L.stream_ptr()))
        assert torch.equal(ar.done(a=a)['a'], R.eot_accumulate(want, None, 1, div))


# ---- FAB's elementwise steps -----------------------------------------------------------------------------------------------------------
FAB_ETA, FAB_BETA = R.f32(1.05), R.f32(0.9)


def _run_fab_update(c):
    L = _lib()
    batch, nps = c['x1'].shape
    ar = Arena()
    x1, x0, d1, d2, al = ar.rw(c['x1']), ar.ro(c['x0']), ar.ro(c['d1']), ar.ro(c['d2']), ar.ro(c['alpha'])
    L.check(L.load().rart_fab_update(L.ptr(x1), L.ptr(x0), L.ptr(d1), L.ptr(d2), L.ptr(al), batch, nps, FAB_ETA, L.stream_ptr()))
    return ar.done(x1=x1)


def _run_fab_backoff(c):
    L = _lib()
    batch, nps = c['x1'].shape
    ar = Arena()
    x1, x0 = ar.rw(c['x1']), ar.ro(c['x0'])
    mask = c['mask'].to(torch.uint8).cuda()
    L.check(L.load().rart_fab_backoff(L.ptr(x1), L.ptr(x0), L.ptr(mask), batch, nps, FAB_BETA, L.stream_ptr()))
    return ar.done(x1=x1)


@SHAPES
def test_fab_update_and_backoff_vs_fp64(batch, nps):
    d = R.inputs(batch, nps)
    x1 = R.start_point(d, 'Linf', R.EPS_LINF)
    alpha = torch.tensor([(0.0, R.f32(0.1), 1.0)[b % 3] for b in range(batch)])
    c = dict(x1=x1, x0=d['x0'], d1=d['u'] * 0.1, d2=d['v'] * 0.1, alpha=alpha)
    got = _run_fab_update(c)
    err = _maxerr(got['x1'], R.fab_update(*R.dbl(c['x1'], c['x0'], c['d1'], c['d2']), alpha, FAB_ETA))
    _report('rart_fab_update', batch, nps, err, 4 * R.ULP1)
    assert err <= 4 * R.ULP1 and _in_box(got['x1'])
    _check_invariances(_run_fab_update, c, got)
    masks = {'off': torch.zeros(batch), 'on': torch.ones(batch), 'mixed': (torch.arange(batch) % 3 != 1).float()}
    for name, mask in masks.items():
        c = dict(x1=x1, x0=d['x0'], mask=mask)
        got = _run_fab_backoff(c)
        err = _maxerr(got['x1'], R.fab_backoff(x1.double(), d['x0'].double(), mask, FAB_BETA))
        _report('rart_fab_backoff ' + name, batch, nps, err, 4 * R.ULP1)
        assert err <= 4 * R.ULP1
        assert R.same_bits(got['x1'][mask == 0], x1[mask == 0])              # masked-off rows untouched
        _check_invariances(_run_fab_backoff, c, got)


def _run_select_rows(c):
    from robustart_amd.noise import adv
    ar = Arena()
    dst, src = ar.rw(c['dst']), ar.ro(c['src'])
    adv.select_rows_(dst, src, c['mask'].bool().cuda())
    return ar.done(dst=dst)


@SHAPES
def test_select_rows(batch, nps):
    d = R.inputs(batch, nps)
    mask = (torch.arange(batch) % 3 != 1).float() if batch > 1 else torch.ones(1)
    c = dict(dst=d['x0'], src=d['g'], mask=mask)
    got = _run_select_rows(c)
    assert R.same_bits(got['dst'], torch.where(mask.view(-1, 1).bool(), d['g'], d['x0']))
    off = _run_select_rows(dict(dst=d['x0'], src=d['g'], mask=torch.zeros(batch)))
    assert R.same_bits(off['dst'], d['x0'])


# ---- one-workgroup-per-row reductions ----------------------------------------------------------------------------------------------------
@SHAPES
def test_row_dot_and_row_norms(batch, nps):
    """rart_row_dot: |got - ref64| <= 2^-23 sum |a_i b_i| (each product is rounded to fp32 before the fp64 sum, the sum once more);
    rart_row_absmax_diff and rart_row_norm_diff Linf: exactly the fp32 maximum of the fp32 differences; L1 / L2: within one fp32 ulp of
    the fp64 norm of the fp32 differences.  Rows span 12 decades: a row that reads its neighbour's sums is far off."""
    L = _lib()
    from robustart_amd.noise import adv
    d = R.inputs(batch, nps)
    ar = Arena()
    a, b, m = ar.ro(d['g']), ar.ro(R.start_point(d, 'L2', R.EPS_L2)), ar.ro(d['g'] * d['m'])
    dot, amax = ar.out(batch), ar.out(batch)
    L.check(L.load().rart_row_dot(L.ptr(a), L.ptr(b), L.ptr(dot), batch, nps, L.stream_ptr()))
    L.check(L.load().rart_row_absmax_diff(L.ptr(a), L.ptr(m), L.ptr(amax), batch, nps, L.stream_ptr()))
    norms = {n: adv.row_norm_diff(a, m, n, out=ar.out(batch)) for n in ('Linf', 'L1', 'L2')}
    got = ar.done(dot=dot, amax=amax, **norms)
    a64, b64 = a.cpu().double(), b.cpu().double()
    ref = (a64 * b64).sum(1)
    bound = R.ULP1 * (a64 * b64).abs().sum(1)
    assert ((got['dot'].double() - ref).abs() <= bound).all(), ((got['dot'].double() - ref).abs() / bound.clamp(min=1e-300)).max()
    _report('rart_row_dot', batch, nps, ((got['dot'].double() - ref).abs() / bound.clamp(min=1e-300)).max().item(), 1.0,
            ' (in units of 2^-23 sum|ab|)')
    diff = d['g'] - d['g'] * d['m']                                  # the fp32 differences
    assert R.same_bits(got['amax'], diff.abs().max(1)[0]) and R.same_bits(got['Linf'], diff.abs().max(1)[0])
    for n, ref in (('L1', diff.double().abs().sum(1)), ('L2', diff.double().pow(2).sum(1).sqrt())):
        ulp = torch.from_numpy(np.spacing(ref.numpy().astype(np.float32)).astype(np.float64))
        e = (got[n].double() - ref).abs()
        _report('rart_row_norm_diff ' + n, batch, nps, (e / ulp).max().item(), 1.0, ' (in fp32 ulps of the norm)')
        assert (e <= ulp).all()


KTH_LENGTHS = (1, 5, 511, 513, 1029)


def _kth_rows(n):
    """rows for the radix select: normal draws; zeros and -0.0; denormals; heavy ties; all equal"""
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(6, n, generator=gen)
    g[1, ::3] = 0.0
    g[1, 1::3] = -0.0
    g[2] = g[2] * 1e-40                                            # denormals: ordered by their bits like every other float
    g[3] = (g[3] * 2).round() / 2                                  # a handful of distinct values
    g[4] = -0.75
    g[5] = g[5] * torch.logspace(-30, 30, n)
    return g


def _kth(g, k):
    L = _lib()
    ar = Arena()
    gg, thr = ar.ro(g), ar.out(g.shape[0])
    kk = torch.as_tensor(k, dtype=torch.int64).cuda()
    L.check(L.load().rart_row_kth_abs(L.ptr(gg), L.ptr(kk), L.ptr(thr), g.shape[0], g.shape[1], L.stream_ptr()))
    return ar.done(thr=thr)['thr']


@pytest.mark.parametrize('n', KTH_LENGTHS)
def test_row_kth_abs_is_exact(n):
    """exactly abs().sort()[k]; k below 0 and above n - 1 is clamped"""
    g = _kth_rows(n)
    for ks in ([0] * 6, [n - 1] * 6, [-1, -5, -(1 << 40), n, n + 7, 1 << 40], [n // 2, n // 3, n // 5, (4 * n) // 5, n // 7, n // 2]):
        k = torch.tensor(ks, dtype=torch.int64)
        assert R.same_bits(_kth(g, k), R.row_kth_abs(g, k)), ks


@pytest.mark.parametrize('n', KTH_LENGTHS)
def test_apgd_l1_move_with_kernel_thresholds(n):
    """delta_u against fp64 within 4 ulp of the largest operand, thresholds from rart_row_kth_abs: ties at the threshold (all of them
    move), a zero-gradient row (count 0: nothing moves), k = 0 (every non-zero entry moves) and k = n - 1 (the largest only)."""
    L = _lib()
    d = R.inputs(6, n, seed=1)
    g = _kth_rows(n)
    g[2] = 0.0                                                      # the zero-gradient row
    g[0, 0] = 0.0
    xa, x0 = torch.clamp(d['x0'] + d['u'] * 0.05, 0, 1), d['x0']
    step = torch.tensor([1.0, 0.25, 0.0625, 1.0, 0.25, 0.0625])
    for ks in ([0] * 6, [n - 1] * 6, [(4 * n) // 5] * 6):
        k = torch.tensor(ks, dtype=torch.int64)
        thr = _kth(g, k)
        assert R.same_bits(thr, R.row_kth_abs(g, k))
        ar = Arena()
        ops = [ar.ro(t) for t in (xa, g, x0, thr, step)]
        du = ar.out(6, n)
        L.check(L.load().rart_apgd_l1_move(*[L.ptr(t) for t in ops], L.ptr(du), 6, n, L.stream_ptr()))
        got = ar.done(du=du)['du']
        want = R.apgd_l1_move(xa.double(), g.double(), x0.double(), thr, step)
        bound = 4 * float(np.spacing(np.float32(max(xa.abs().max().item(), x0.abs().max().item(), step.max().item()))))
        err = _maxerr(got, want)
        _report('rart_apgd_l1_move', 6, n, err, bound, ' k = %d' % ks[0])
        assert err <= bound
        assert R.same_bits(got[2], xa[2] - x0[2])                  # count 0: x_adv - x0, nothing added
        moved = got != (xa - x0)
        sel = (g.abs() >= thr.view(-1, 1)) & (g != 0)
        assert not (moved & ~sel).any()                             # nothing below the threshold moves
        if ks[0] == n - 1:
            assert sel[3].sum() >= 1 and (sel[4].sum() == n)        # ties at the threshold are all selected
        if ks[0] == 0:
            assert sel[0].sum() == (g[0] != 0).sum()


# ---- the exact L1 projection on short rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 5, 513])
def test_l1_project_short_rows_vs_fp64(n):
    """rows shorter than the 512-thread workgroup and just above it, against A.l1_projection in double: a row inside the ball (delta = 0),
    rows that need the projection (they land on the sphere to 2e-6 eps), a row where the box shrink alone suffices; delta to 1e-4 as at
    ImageNet row length; both point_out settings."""
    from robustart_amd.noise import adv
    gen = torch.Generator().manual_seed(n)
    eps = R.f32(0.15 * n)
    x = 0.2 + 0.6 * torch.rand(5, n, generator=gen)
    sgn = torch.where(torch.rand(5, n, generator=gen) < 0.5, -1.0, 1.0)
    y = sgn * (0.2 + 0.4 * torch.rand(5, n, generator=gen))       # rows 1, 3, 4: sum |y| >= 0.2 n > eps: projected
    y[0] = sgn[0] * 0.05 * torch.rand(n, generator=gen)            # row 0: inside the ball and the box
    x[2], y[2] = 0.9, 0.3                                           # row 2: the box takes 0.2 per coordinate, 0.1 n <= eps is left
    y[4] = y[4] * 3                                                 # row 4: far outside the box as well
    want = A.l1_projection(x.double(), y.double(), eps)
    if n == 1:
        # One coordinate: the oracle's search over sorted breakpoints (a restatement of the reference's, which has the same limit) reads
        # past its only interior breakpoint and returns the box shrink alone for rows that need the projection -- outside the ball it
        # promises.  The projection of one coordinate is closed-form: |y| shrinks by clip(|y| - eps, lo, |y|).  Rows 0 and 2, which need
        # no projection, still come from the oracle.
        x64, y64 = x.double(), y.double()
        lo = -torch.clamp(torch.min(1 - x64 - y64, x64 + y64), max=0.0)
        closed = -y64.sign() * torch.min(torch.max(y64.abs() - eps, lo), y64.abs())
        assert torch.equal(closed[[0, 2]], want[[0, 2]]) and ((y64 + want).abs().sum(1)[[1, 3, 4]] > eps * 1.2).all()
        want = closed
    assert (want[0] == 0).all() and torch.allclose(want[2], torch.full((n,), -0.2, dtype=torch.float64), atol=1e-7)
    ar = Arena()
    xg, yg = ar.ro(x), ar.ro(y)
    delta = adv.l1_projection(xg, yg, eps, out=ar.out(5, n))
    point = adv.l1_projection(xg, yg, eps, point_out=True, out=ar.out(5, n))
    clamped = adv.l1_projection(xg, yg, eps, point_out=True, clamp01=True, out=ar.out(5, n))
    got = ar.done(delta=delta, point=point, clamped=clamped)
    err = _maxerr(got['delta'], want)
    _report('rart_l1_project', 5, n, err, 1e-4)
    assert err <= 1e-4 and (got['delta'][0] == 0).all()
    spent = (y.double() + got['delta'].double()).abs().sum(1)
    assert ((spent[[1, 3, 4]] - eps).abs() <= 2e-6 * eps).all(), spent
    assert spent[2] <= eps and spent[0] <= eps
    z = x.double() + y.double() + got['delta'].double()
    assert z.min() >= -1e-6 and z.max() <= 1 + 1e-6
    assert _maxerr(got['point'], x.double() + y.double() + want) <= 1e-4
    assert R.same_bits(got['point'], (x + y) + got['delta']) and R.same_bits(got['clamped'], torch.clamp(got['point'], 0, 1))
