"""HIP training-side step kernels vs the oracle (oracle/train_ref.py, pinned to torch.optim in the CPU suite): small arenas, arenas
beyond the size at which the launch stops growing (the grid-stride loop), AdamW with the switches HipOptimizer.step sets, the EMA kernel
on its own, and HipOptimizer over an arena with a no-decay range."""
import numpy as np
import pytest
import torch

from oracle import train_ref as T

pytestmark = pytest.mark.gpu


def _lib():
    from robustart_amd import _lib
    return _lib, _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rand(n, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(n) * scale).astype(np.float32)


@pytest.mark.parametrize('n', [4, 1027, 262147])
@pytest.mark.parametrize('nesterov,wd,ema', [(1, 1e-4, True), (0, 0.0, False)])
def test_sgd_step_kernel_matches_oracle(n, nesterov, wd, ema):
    L, lib = _lib()
    p, m = _rand(n, 0), np.zeros(n, np.float32)
    e = p.copy()
    dp, dm, de = _dev(p), _dev(m), _dev(e)
    for step in range(3):
        g = _rand(n, 10 + step, 0.05)
        dg = _dev(g)
        lr, scale = 0.1 + 0.1 * step, 0.5
        L.check(lib.rart_sgd_step_f32(dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), de.data_ptr() if ema else None, n, lr,
                                      0.9, wd, nesterov, scale, 0.999, 1, L.stream_ptr()))
        p, m = T.sgd_step(p, g, m, lr, 0.9, wd, bool(nesterov), grad_scale=scale)
        e = T.ema_update(e, p, 0.999)
        torch.cuda.synchronize()
        assert torch.count_nonzero(dg).item() == 0                      # fused gradient reset
        np.testing.assert_array_equal(dp.cpu().numpy(), p)              # op-by-op fp32: bit exact
        np.testing.assert_array_equal(dm.cpu().numpy(), m)
        if ema:
            np.testing.assert_array_equal(de.cpu().numpy(), e)


@pytest.mark.parametrize('n', [5, 40003])
def test_adamw_step_kernel_matches_oracle(n):
    L, lib = _lib()
    p, m, v = _rand(n, 1), np.zeros(n, np.float32), np.zeros(n, np.float32)
    dp, dm, dv = _dev(p), _dev(m), _dev(v)
    for step in range(1, 5):
        g = _rand(n, 20 + step, 0.02)
        dg = _dev(g)
        L.check(lib.rart_adamw_step_f32(dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), None, n, 1e-3, 0.9,
                                        0.999, 1e-8, 0.05, step, 1.0, 0.0, 0, L.stream_ptr()))
        p, m, v = T.adamw_step(p, g, m, v, 1e-3, step, 0.9, 0.999, 1e-8, 0.05)
        torch.cuda.synchronize()
        assert torch.equal(dg.cpu(), torch.from_numpy(g))               # zero_grad = 0 leaves the gradient alone
        np.testing.assert_allclose(dp.cpu().numpy(), p, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(dv.cpu().numpy(), v, rtol=1e-6, atol=1e-14)


def test_optimizer_argument_checks():
    L, lib = _lib()
    t = torch.zeros(16, device='cuda')
    assert lib.rart_sgd_step_f32(None, t.data_ptr(), t.data_ptr(), None, 16, 0.1, 0.9, 0.0, 1, 1.0, 0.0, 1, None) != 0
    assert lib.rart_sgd_step_f32(t.data_ptr(), t.data_ptr(), t.data_ptr(), None, 16, 0.1, 0.0, 0.0, 1, 1.0, 0.0, 1,
                                 None) != 0                                # nesterov without momentum (torch raises too)
    assert lib.rart_adamw_step_f32(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), None, 16, 1e-3, 0.9, 0.999,
                                   1e-8, 0.0, 0, 1.0, 0.0, 0, None) != 0   # step counts from 1


@pytest.mark.parametrize('batch,classes,s', [(1, 10, 0.0), (7, 1000, 0.1), (256, 1000, 0.1), (5, 63, 0.3)])
def test_label_smooth_ce_kernel(batch, classes, s):
    from robustart_amd.train.arena import label_smooth_ce
    rs = np.random.RandomState(batch)
    z = (rs.standard_normal((batch, classes)) * 4).astype(np.float32)
    y = rs.randint(0, classes, batch)
    loss, dl = label_smooth_ce(_dev(z), _dev(y.astype(np.int64)), s, 1.0 / batch)
    ref_loss, ref_grad = T.label_smooth_ce(z, y, s, 1.0 / batch)
    np.testing.assert_allclose(loss.cpu().numpy(), ref_loss, rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(dl.cpu().numpy(), ref_grad, rtol=2e-5, atol=2e-9)
    # and against torch on the GPU
    zt = _dev(z).requires_grad_(True)
    lt = torch.nn.functional.cross_entropy(zt, _dev(y.astype(np.int64)), label_smoothing=s, reduction='none')
    (lt.sum() / batch).backward()
    np.testing.assert_allclose(loss.cpu().numpy(), lt.detach().cpu().numpy(), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(dl.cpu().numpy(), zt.grad.cpu().numpy(), rtol=2e-5, atol=2e-9)


def test_solver_train_hip_optimizer_tracks_torch_scaffold():
    """3 iterations of cls_solver.train on a tiny model: HIP loss/optimizer/EMA path vs torch.optim on the same arena."""
    import robustart_amd.model as M
    from robustart_amd.train import cls_solver as S

    def tiny(**kw):
        torch.manual_seed(0)
        return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, stride=4), torch.nn.BatchNorm2d(8), torch.nn.ReLU(),
                                   torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), torch.nn.Linear(8, 1000))
    M._REGISTRY['tiny_bn_test'] = tiny

    class Args:
        pass
    outs = {}
    for engine in ('hip', 'torch'):
        args = Args()
        args.engine, args.max_iter = engine, 3
        cfg = {'model': {'type': 'tiny_bn_test'}, 'data': {'fake_size': 16, 'batch_size': 8, 'input_size': 32},
               'label_smooth': 0.1, 'ema': {'enable': True, 'kwargs': {'decay': 0.9}}, 'max_iter': 3, 'bf16': False,
               'optimizer': {'type': 'SGD', 'no_wd': {'norm': True},
                             'kwargs': {'nesterov': True, 'momentum': 0.9, 'weight_decay': 1e-2}},
               'lr_scheduler': {'kwargs': {'base_lr': 0.05, 'warmup_lr': 0.1}}}
        loss, model = S.train(cfg, args, 0, 1, torch.device('cuda'))
        outs[engine] = (loss, torch.cat([p.detach().flatten() for p in model.parameters()]).cpu())
    assert abs(outs['hip'][0] - outs['torch'][0]) < 1e-4
    np.testing.assert_allclose(outs['hip'][1].numpy(), outs['torch'][1].numpy(), rtol=1e-4, atol=1e-6)


# ---- beyond the launch cap, with every switch HipOptimizer.step uses, and rart_ema_update_f32 on its own ----
# grid_for (csrc/train_steps.hip) stops growing at 256 * 32 workgroups of 256 threads; a thread of the step kernels owns a float4, a thread
# of the EMA kernel one float.  Beyond that the kernels grid-stride, which is where every real arena (25 - 90 M floats) runs.
CAP_THREADS = 256 * 32 * 256
N_ABOVE = CAP_THREADS * 4 + 4099         # 1 024 float4 for the second trip of the loop, then a 3-element tail


def _one_signed(n, seed, scale):
    """Gradients in [0.5, inf) * scale: none is zero, so an element the kernel skipped keeps a non-zero gradient, and all are positive and
    larger than the weight-decay term, so both SGD and AdamW move every parameter down at every step (AdamW: the step is lr at step 1
    and at least 0.67 lr at step 2 for two positive gradients, against a decay of lr * wd * |p| < 0.3 lr) and none can return to its
    initial value."""
    return ((0.5 + np.abs(np.random.RandomState(seed).standard_normal(n))) * scale).astype(np.float32)


def test_sgd_step_kernel_above_the_launch_cap():
    L, lib = _lib()
    n = N_ABOVE
    assert n // 4 > CAP_THREADS and n % 4 != 0
    p0 = _rand(n, 0)
    p, m, e = p0.copy(), np.zeros(n, np.float32), p0.copy()
    dp, dm, de = _dev(p), _dev(m), _dev(e)
    for step in range(2):
        g = _one_signed(n, 10 + step, 0.05)
        assert np.count_nonzero(g) == n
        dg = _dev(g)
        lr, scale = 0.1 + 0.1 * step, 0.5
        L.check(lib.rart_sgd_step_f32(dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), de.data_ptr(), n, lr, 0.9, 1e-4, 1, scale, 0.999, 1,
                                      L.stream_ptr()))
        p, m = T.sgd_step(p, g, m, lr, 0.9, 1e-4, True, grad_scale=scale)
        e = T.ema_update(e, p, 0.999)
        assert torch.count_nonzero(dg).item() == 0                      # every gradient was reset: no element was skipped
        np.testing.assert_array_equal(dp.cpu().numpy(), p)              # op-by-op fp32: bit exact
        np.testing.assert_array_equal(dm.cpu().numpy(), m)
        np.testing.assert_array_equal(de.cpu().numpy(), e)
    assert int((dp.cpu().numpy() == p0).sum()) == 0                     # every parameter moved


def test_adamw_step_kernel_above_the_launch_cap():
    L, lib = _lib()
    n = N_ABOVE
    p0 = _rand(n, 1)
    p, m, v, e = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32), p0.copy()
    dp, dm, dv, de = _dev(p), _dev(m), _dev(v), _dev(e)
    for step in (1, 2):
        g = _one_signed(n, 20 + step, 0.02)
        assert np.count_nonzero(g) == n
        dg = _dev(g)
        L.check(lib.rart_adamw_step_f32(dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), de.data_ptr(), n, 1e-3, 0.9, 0.999,
                                        1e-8, 0.05, step, 1.0, 0.9999, 1, L.stream_ptr()))
        p, m, v = T.adamw_step(p, g, m, v, 1e-3, step, 0.9, 0.999, 1e-8, 0.05)
        e = T.ema_update(e, p, 0.9999)
        assert torch.count_nonzero(dg).item() == 0
        np.testing.assert_allclose(dp.cpu().numpy(), p, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(dm.cpu().numpy(), m, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(dv.cpu().numpy(), v, rtol=1e-6, atol=1e-14)
        np.testing.assert_allclose(de.cpu().numpy(), e, rtol=1e-6, atol=1e-8)
    assert int((dp.cpu().numpy() == p0).sum()) == 0


@pytest.mark.parametrize('n', [5, 40003])
def test_adamw_step_kernel_with_ema_grad_scale_and_gradient_reset(n):
    """the switches HipOptimizer.step always sets: ema != NULL, zero_grad = 1, grad_scale != 1"""
    L, lib = _lib()
    p, m, v = _rand(n, 1), np.zeros(n, np.float32), np.zeros(n, np.float32)
    e = p.copy()
    dp, dm, dv, de = _dev(p), _dev(m), _dev(v), _dev(e)
    for step in range(1, 5):
        g = _rand(n, 20 + step, 0.02)
        dg = _dev(g)
        L.check(lib.rart_adamw_step_f32(dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), de.data_ptr(), n, 1e-3, 0.9, 0.999,
                                        1e-8, 0.05, step, 0.5, 0.9999, 1, L.stream_ptr()))
        p, m, v = T.adamw_step(p, g * np.float32(0.5), m, v, 1e-3, step, 0.9, 0.999, 1e-8, 0.05)
        e = T.ema_update(e, p, 0.9999)
        assert torch.count_nonzero(dg).item() == 0
        np.testing.assert_allclose(dp.cpu().numpy(), p, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(dv.cpu().numpy(), v, rtol=1e-6, atol=1e-14)
        np.testing.assert_allclose(de.cpu().numpy(), e, rtol=1e-6, atol=1e-8)           # the tolerance p has


@pytest.mark.parametrize('n', [1, 1027, CAP_THREADS + 4099])
def test_ema_update_kernel_matches_oracle(n):
    """bit-exact: the oracle's ema_update is op-by-op fp32 (decay * ema + fp32(1 - decay) * p, the difference formed in double and
    rounded once) and the kernel is compiled without FMA contraction, as for SGD"""
    L, lib = _lib()
    e = _rand(n, 40)
    de = _dev(e)
    for step in range(2):
        p = _rand(n, 41 + step)
        dp = _dev(p)
        L.check(lib.rart_ema_update_f32(de.data_ptr(), dp.data_ptr(), n, 0.9999, L.stream_ptr()))
        e = T.ema_update(e, p, 0.9999)
        np.testing.assert_array_equal(de.cpu().numpy(), e)
        assert torch.equal(dp.cpu(), torch.from_numpy(p))               # the parameters are read only


def test_hip_optimizer_adamw_with_two_weight_decay_ranges():
    """HipOptimizer over a ParamArena whose norm / bias parameters sit in the no-decay range: two launches per step, each with its own
    weight decay; every arena element against the oracle applied per range, the padding between parameters exactly 0"""
    from robustart_amd.train.arena import HipOptimizer, ParamArena
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.LayerNorm(7), torch.nn.Linear(7, 3)).cuda()
    arena = ParamArena(model, no_decay=lambda name, p: p.dim() == 1)
    n, end = arena.numel, arena.decay_end
    assert [p.numel() for p in arena.params] == [35, 21, 7, 7, 7, 3] and 0 < end < n and n > sum(p.numel() for p in arena.params)
    pad = np.ones(n, bool)
    for p, o in zip(arena.params, arena.offsets):
        pad[o:o + p.numel()] = False
    assert pad.sum() == 8
    lr, wd, decay, scale = 1e-3, 0.05, 0.9999, 0.5
    opt = HipOptimizer(arena, kind='AdamW', lr=lr, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8, ema_decay=decay)
    p = arena.flat_p.cpu().numpy().copy()
    m, v, e = np.zeros(n, np.float32), np.zeros(n, np.float32), p.copy()
    gen = torch.Generator().manual_seed(1)
    for step in (1, 2):
        for q in arena.params:
            q.grad.copy_(0.02 * torch.randn(q.shape, generator=gen))
        g = arena.flat_g.cpu().numpy().copy()
        assert not g[pad].any()
        opt.step(grad_scale=scale)
        for lo, hi, w in ((0, end, wd), (end, n, 0.0)):
            p[lo:hi], m[lo:hi], v[lo:hi] = T.adamw_step(p[lo:hi], g[lo:hi] * np.float32(scale), m[lo:hi], v[lo:hi], lr, step, 0.9, 0.999,
                                                        1e-8, w)
        e = T.ema_update(e, p, decay)
        assert torch.count_nonzero(arena.flat_g).item() == 0
        for got, want, atol in ((arena.flat_p, p, 1e-8), (opt.m, m, 1e-8), (opt.v, v, 1e-14), (opt.ema, e, 1e-8)):
            got = got.cpu().numpy()
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=atol)
            assert not got[pad].any()                                   # padding stays exactly 0
    for q, o in zip(arena.params, arena.offsets):                        # the module's parameters are the arena's elements
        assert q.data_ptr() == arena.flat_p.data_ptr() + 4 * o
