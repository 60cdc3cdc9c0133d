"""CPU checks of tests/_attack_steps_ref.py, the references tests/test_attack_step_kernels_gpu.py holds csrc/attack_steps.hip to:
the host mirror of the native draws cannot drift from the generator that is already tested, every tolerance of the GPU suite is
reached by a correct fp32 implementation (the fp32 oracle against the fp64 restatement, on the same inputs), and the share of
elements the MIM comparison may skip stays under its cap for the reference alone."""
import numpy as np
import pytest
import torch

import _attack_steps_ref as R
from oracle import attacks_ref as A
from robustart_amd.noise import rng

CPU_ROWS = (1, 31, 33, 257, R.IMAGENET_ROW)
CPU_SHAPES = [(b, n) for n in CPU_ROWS[:-1] for b in R.BATCHES] + [(7, R.IMAGENET_ROW)]


def test_word_mirror_is_the_tested_generator():
    """words() is rng.threefry2x32 on numpy lanes: every 32-bit word equals the scalar call, and the 53 bits host_uniform keeps of a
    word pair reproduce rng.host_uniform for the same (seed, sample, stream, index) -- streams 1, 3, 5 of the kernels and a host one."""
    seeds = (0, 5, 1234567, (0xDEADBEEF << 32) | 0x12345678)
    samples = [0, 1, 100, 104, (1 << 32) - 1]
    counters = [0, 1, 2, 75263, 0xFFFFFFF]
    for seed in seeds:
        for stream in (1, 3, 5, 11):
            w0, w1 = R.words(seed, samples, stream, counters)
            assert w0.shape == (len(samples), len(counters)) and int(w0.max()) < 1 << 32 and int(w1.max()) < 1 << 32
            for i, smp in enumerate(samples):
                for j, c in enumerate(counters):
                    want = rng.threefry2x32(seed & 0xFFFFFFFF, seed >> 32, rng.ctr0(c, stream), smp)
                    assert (int(w0[i, j]), int(w1[i, j])) == want
                    u = ((int(w0[i, j]) >> 5) * 67108864.0 + (int(w1[i, j]) >> 6)) / 9007199254740992.0
                    assert u == rng.host_uniform(seed, smp, stream, c)


def test_native_draw_mirrors_follow_the_kernels_mapping():
    """native_pm1: element e reads counter e >> 1 of stream 1, .x for even e and .y for odd; values in (-1, 1) on the fp32 grid of
    u01; Square's stripe signs: stream 3, counter c * W + w, low bit of .x; the L1 start: stream 5, counter e, radius at 0xFFFFFFF."""
    seed, samples = 77, R.row_samples(3, sample_offset=9)
    assert samples.tolist() == [9, 10, 11] and R.row_samples(3, rows=[5, 2, 9]).tolist() == [5, 2, 9]
    pm = R.native_pm1(seed, samples, 7)
    assert pm.shape == (3, 7) and pm.dtype == torch.float32 and pm.abs().max() <= 1
    for b, smp in enumerate(samples.tolist()):
        for e in range(7):
            w = rng.threefry2x32(seed, 0, rng.ctr0(e >> 1, 1), smp)[e & 1]
            want = np.float32(2) * ((np.float32(w >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)) - np.float32(1)
            assert pm[b, e].item() == float(want)
    assert R.u01(0xFFFFFFFF) == np.float32(1.0) and R.u01(0) == np.float32(2.0 ** -25)       # the ends of the grid, rounded as fp32 does
    sg = R.native_square_signs(seed, samples, 3, 5)
    for b, smp in enumerate(samples.tolist()):
        for c in range(3):
            for w in range(5):
                assert sg[b, c, w].item() == (1.0 if rng.threefry2x32(seed, 0, rng.ctr0(c * 5 + w, 3), smp)[0] & 1 else -1.0)
    se, rad = R.native_l1_start_draws(seed, samples, 4, 2.0)
    for b, smp in enumerate(samples.tolist()):
        for e in range(4):
            wx, wy = rng.threefry2x32(seed, 0, rng.ctr0(e, 5), smp)
            assert (se[b, e].item() < 0) == bool(wy & 1) and abs(se[b, e].item()) == -np.log(np.float64(R.u01(wx)))
        assert rad[b].item() == np.sqrt(np.float64(R.u01(rng.threefry2x32(seed, 0, rng.ctr0(0xFFFFFFF, 5), smp)[1])) * 4.0)
    # a larger row through the vectorised path only: mean and spread of a uniform (-1, 1)
    big = R.native_pm1(3, R.row_samples(2, 100), 150528)
    assert abs(big.mean().item()) < 5e-3 and abs(big.std().item() - 1 / np.sqrt(3)) < 5e-3


@pytest.mark.parametrize('batch,nps', [(1, 1), (3, 3), (7, 33), (3, 257)])
def test_input_builder_properties(batch, nps):
    d = R.build_inputs(batch, nps)
    assert all(v.shape[0] == batch and v.dtype == torch.float32 for v in d.values())
    if batch > 1:
        absmax = d['g'].abs().max(1)[0]
        live = [b for b in range(batch) if not (batch >= 3 and b == R.DEAD_ROW)]
        assert absmax[live[-1]] / absmax[live[0]] > 1e8 or nps < 3                      # rows of very different norms
    if batch >= 3:
        assert (d['g'][R.DEAD_ROW] == 0).all()
        assert (d['ratio'] == R.RATIO_OUT).any() and (d['ratio'] == R.RATIO_IN).any()
    if nps >= 7:
        assert (d['x0'] == 0.0).any() and (d['x0'] == 1.0).any()
        g0 = d['g'][0]
        assert ((g0 == 0) & ~torch.signbit(g0)).any() and ((g0 == 0) & torch.signbit(g0)).any()      # 0.0 and -0.0
    for norm, eps in (('Linf', R.EPS_LINF), ('L2', R.EPS_L2), ('L1', R.eps_l1(nps))):
        x = R.start_point(d, norm, eps)
        dd = (x.double() - d['x0'].double())
        n = dd.abs().max(1)[0] if norm == 'Linf' else (dd.abs().sum(1) if norm == 'L1' else dd.pow(2).sum(1).sqrt())
        out = d['ratio'] > 1
        if norm == 'Linf':
            if nps >= 33:
                assert (n[out] > eps).all()
            assert (n[~out] <= eps * (1 + 1e-6)).all()
            if nps >= 9:
                e = torch.tensor(eps)
                assert torch.equal(x[:, 0], (d['x0'] + e)[:, 0]) and torch.equal(x[:, 5], (d['x0'] - e)[:, 5])
        else:
            assert (n[out] > 1.4 * eps).all() and (n[~out] < 0.6 * eps).all()


def _err(a32, b64):
    return (a32.double() - b64).abs().max().item()


@pytest.mark.parametrize('batch,nps', CPU_SHAPES)
def test_fp32_oracles_reach_the_gpu_tolerances(batch, nps):
    """The fp32 oracle (the same torch expression in fp32) against the fp64 restatement, on the very inputs and with the very bounds
    of the GPU suite: 1e-6 PGD-L2 and MIM, 2e-6 APGD-L2, 1e-7 the APGD starts.  Both branches of min(eps / |d|, 1) are taken."""
    d = R.inputs(batch, nps)
    c = R.step_case('pgd_l2', batch, nps)
    w32 = R.pgd_l2_step(c['x'], c['g'], c['x0'], R.EPS_L2, R.PGD_L2_ALPHA)
    w64 = R.pgd_l2_step(*R.dbl(c['x'], c['g'], c['x0']), R.EPS_L2, R.PGD_L2_ALPHA)
    e_l2 = _err(w32, w64)
    assert e_l2 <= 1e-6 and w64.min() >= 0 and w64.max() <= 1
    x64, g64, x064 = R.dbl(c['x'], c['g'], c['x0'])
    dn = (x64 + R.PGD_L2_ALPHA * g64 / g64.pow(2).sum(1, keepdim=True).sqrt().clamp(min=1e-12) - x064).pow(2).sum(1).sqrt()
    assert (dn[d['ratio'] > 1] > R.EPS_L2).all() and (dn[d['ratio'] < 1] < R.EPS_L2).all()      # factor < 1 and factor = 1
    errs = {'pgd_l2': e_l2}
    for norm in ('Linf', 'L2'):
        c = R.step_case('apgd_' + norm, batch, nps)
        eps = R.EPS_LINF if norm == 'Linf' else R.EPS_L2
        for a in (1.0, 0.75):
            w32 = R.apgd_step(c['xa'], c['xold'], c['g'], c['x0'], eps, c['step'], a, norm)
            w64 = R.apgd_step(*R.dbl(c['xa'], c['xold'], c['g'], c['x0']), eps, c['step'], a, norm)
            e = _err(w32, w64)
            errs['apgd_%s_%g' % (norm, a)] = e
            # Linf: elementwise, no discontinuity (sign(grad) is exact, clamps are 1-Lipschitz): 5 roundings of values below 2
            assert e <= (4 * R.ULP1 if norm == 'Linf' else 2e-6)
    for norm, t in (('Linf', d['t_uniform']), ('L2', d['t_normal']), ('L1', d['t_normal'])):
        eps = {'Linf': R.EPS_LINF, 'L2': R.EPS_L2, 'L1': R.eps_l1(nps)}[norm]
        e = _err(R.apgd_start(d['x0'], t, norm, eps), R.apgd_start(d['x0'].double(), t.double(), norm, eps))
        errs['start_' + norm] = e
        assert e <= 1e-7
    print('fp32 oracle vs fp64 at %d x %d: %s' % (batch, nps, ' '.join('%s %.2e' % kv for kv in sorted(errs.items()))))


@pytest.mark.parametrize('batch,nps', CPU_SHAPES)
def test_l1_bounds_are_small_and_finite(batch, nps):
    """The PGD-L1 step and the injected L1 start have no earlier direct test: their GPU bound is 8 x the fp32 restatement's own error
    + one ulp at 1.0 (R.l1_bound).  Here: that error is a rounding error (below 1e-6), so the bound cannot hide a wrong kernel."""
    c = R.step_case('pgd_l1', batch, nps)
    eps = R.eps_l1(nps)
    w64 = R.pgd_l1_step(*R.dbl(c['x'], c['g'], c['x0']), eps, eps / 8)
    e1 = _err(R.pgd_l1_step(c['x'], c['g'], c['x0'], eps, eps / 8), w64)
    assert (w64 - c['x0'].double()).abs().sum(1).max() <= eps * (1 + 1e-9) and w64.min() >= 0 and w64.max() <= 1
    c = R.step_case('l1_start', batch, nps)
    e2 = _err(R.l1_sphere_start(c['x0'], c['se'], c['radius']), R.l1_sphere_start(*R.dbl(c['x0'], c['se'], c['radius'])))
    print('L1 fp32 restatement vs fp64 at %d x %d: step %.2e (bound %.2e) start %.2e (bound %.2e)'
          % (batch, nps, e1, R.l1_bound(e1), e2, R.l1_bound(e2)))
    assert e1 < 1e-6 and e2 < 1e-6


def test_pgd_l1_restatement_is_the_oracles_step():
    """R.pgd_l1_step in fp32 == one iteration of A.pgd_l1_art (the restatement of ART the attack-level test uses) to fp32 rounding"""
    c = R.step_case('pgd_l1', 3, 257)
    eps = R.eps_l1(257)
    se = np.zeros((3, 257), np.float32)
    se[:, 0] = 1.0
    x = np.clip(c['x'].numpy(), 0, 1)                  # the oracle starts from its own clipped start: feed it a fixed point of that
    got = A.pgd_l1_art(lambda xa, y: c['g'].numpy(), x, None, eps, eps / 8, 1, se, np.zeros(3, np.float32))
    # pgd_l1_art measures delta against its input x, so restate with x0 = x
    want = R.pgd_l1_step(torch.from_numpy(x).double(), c['g'].double(), torch.from_numpy(x).double(), eps, eps / 8)
    assert np.abs(got.astype(np.float64) - want.numpy()).max() <= 2 * R.ULP1


@pytest.mark.parametrize('batch,nps', R.SHAPES)
def test_mim_exclusion_cap_holds_for_the_reference(batch, nps):
    """At most MIM_EXCLUDE_CAP of a tensor's elements have an fp64 momentum below MIM_M_EXCLUDE (where fp32 may pick the other sign),
    on every input the GPU test uses; away from them the fp32 oracle is within 1e-6 of fp64 (x) and 1e-5 relative (momentum)."""
    c = R.step_case('mim', batch, nps)
    live = [b for b in range(batch) if not (batch >= 3 and b == R.DEAD_ROW)]          # the reference divides by zero on the dead row
    x, m, g, x0 = (c[k][live] for k in ('x', 'm', 'g', 'x0'))
    wx, wm = R.mim_step(*R.dbl(x, g, m, x0), R.EPS_LINF, R.MIM_STEP, R.MIM_DECAY)
    skip = wm.abs() < R.MIM_M_EXCLUDE
    assert skip.sum().item() <= R.MIM_EXCLUDE_CAP * wm.numel(), (skip.sum().item(), wm.numel())
    fx, fm = R.mim_step(x, g, m, x0, R.EPS_LINF, R.MIM_STEP, R.MIM_DECAY)
    assert ((fx.double() - wx).abs()[~skip] <= 1e-6).all()
    assert ((fm.double() - wm).abs() <= 1e-5 + 1e-5 * wm.abs()).all()
    assert torch.isfinite(wx).all() and wx.min() >= 0 and wx.max() <= 1


def test_l1_projection_oracle_keeps_fp64():
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(4, 513, generator=g), torch.randn(4, 513, generator=g) * 0.1
    d64 = A.l1_projection(x.double(), y.double(), 2.0)
    assert d64.dtype == torch.float64 and A.l1_projection(x, y, 2.0).dtype == torch.float32
    assert (d64 - A.l1_projection(x, y, 2.0).double()).abs().max() < 1e-5
    spent = (y.double() + d64).abs().sum(1)
    assert ((spent - 2.0).abs() <= 1e-12).all()                        # on the sphere to fp64 rounding, which fp32 cannot give
