"""Mixup / CutMix on the GPU: rart_mix_batch_f32 against the torch expressions it replaces (bit for bit), rart_label_smooth_ce_mix_f32
against the one-label entry and fp64 autograd, and one solver step per train engine on a mixed batch."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SENTINEL = -7.0


# ---- rart_mix_batch_f32 -------------------------------------------------------------------------------------------------------------------
_SOURCES = {}


def _sources(n, h, w):
    """(u8 NHWC, fp32 NCHW, perm) of a shape, made once"""
    key = (n, h, w)
    if key not in _SOURCES:
        g = torch.Generator().manual_seed(n * 1000 + h)
        u8 = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).cuda()
        f32 = torch.rand(n, 3, h, w, generator=g).cuda()
        perm = np.array([0, 2, 1]) if n == 3 else np.random.default_rng(n).permutation(n)
        _SOURCES[key] = (u8, f32, perm)
    return _SOURCES[key]


def _launch(src, perm, mode, lam, box, pad=64):
    """the entry itself, dst inside a larger buffer of sentinels (pad floats on either side) that must survive"""
    from robustart_amd import _lib as L
    is_u8 = src.dtype == torch.uint8
    n, h, w = (src.shape[0], src.shape[1], src.shape[2]) if is_u8 else (src.shape[0], src.shape[2], src.shape[3])
    elems = n * 3 * h * w
    buf = torch.full((elems + 2 * pad,), SENTINEL, dtype=torch.float32, device='cuda')
    pd = torch.from_numpy(np.asarray(perm).astype(np.int32)).cuda()
    y0, y1, x0, x1 = box if box is not None else (0, 0, 0, 0)
    L.check(L.load().rart_mix_batch_f32(src.data_ptr(), 1 if is_u8 else 0, pd.data_ptr(), buf.data_ptr() + 4 * pad, n, h, w, mode,
                                        float(lam), y0, y1, x0, x1, L.stream_ptr()))
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + elems:] == SENTINEL).all()), 'a store left dst'
    return buf[pad:pad + elems].view(n, 3, h, w)


def _want(src, perm, mode, lam, box):
    """the torch expressions on the device"""
    x01 = src.permute(0, 3, 1, 2).float().div(255.0) if src.dtype == torch.uint8 else src
    idx = torch.from_numpy(np.asarray(perm).astype(np.int64)).cuda()
    if mode == 1:
        return lam * x01 + (1.0 - lam) * x01[idx]
    y0, y1, x0, x1 = box
    out = x01.clone()
    out[:, :, y0:y1, x0:x1] = x01[idx][:, :, y0:y1, x0:x1]
    return out


def _boxes(h, w):
    return [(0, 0, 0, 0), (h // 2, h // 2, w // 2, w // 2), (0, h, 0, w),                           # empty (twice), full image
            (0, h // 2, 1, w - 1), (h // 2, h, 1, w - 1), (1, h - 1, 0, w // 2), (1, h - 1, w // 2, w),   # touching each border
            (1, h - 1, 1, w - 2), (2, 3, 5, 6), (1, h - 2, 3, w - 3), (0, h, 2, 3)]                  # x0, x1 no multiples of 4


SHAPES = [(3, 8, 12), (5, 6, 10), (2, 224, 224)]


@pytest.mark.parametrize('is_u8', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_mixup_is_the_torch_expression_bit_for_bit(shape, is_u8):
    u8, f32, perm = _sources(*shape)
    src = u8 if is_u8 else f32
    beta = float(np.random.default_rng(1).beta(0.2, 0.2))
    for lam in (0.0, 1.0, 0.5, beta, 0.2871):
        assert torch.equal(_launch(src, perm, 1, lam, None), _want(src, perm, 1, lam, None)), lam
    # lam = 1 is the hand-over itself
    assert torch.equal(_launch(src, perm, 1, 1.0, None), u8.permute(0, 3, 1, 2).float().div(255.0) if is_u8 else f32)


@pytest.mark.parametrize('is_u8', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_cutmix_is_the_torch_expression_bit_for_bit(shape, is_u8):
    u8, f32, perm = _sources(*shape)
    src = u8 if is_u8 else f32
    for box in _boxes(shape[1], shape[2]):
        assert torch.equal(_launch(src, perm, 2, 0.5, box), _want(src, perm, 2, 0.5, box)), box


@pytest.mark.parametrize('is_u8', [True, False])
def test_a_batch_past_the_grid_cap_takes_a_second_trip_of_the_stride_loop(is_u8):
    """4096 blocks of 256 threads: 90 images of 224 x 224 are 1 128 960 four-pixel items (u8) or 3 386 880 float4 items (fp32)"""
    n, h, w = 90, 224, 224
    u8, f32, perm = _sources(n, h, w)
    src = u8 if is_u8 else f32
    assert n * h * (w // 4) > 4096 * 256
    assert torch.equal(_launch(src, perm, 1, 0.2871, None), _want(src, perm, 1, 0.2871, None))
    box = (17, 201, 30, 163)
    assert torch.equal(_launch(src, perm, 2, 0.5, box), _want(src, perm, 2, 0.5, box))


@pytest.mark.parametrize('is_u8', [True, False])
def test_a_dst_offset_by_four_bytes_takes_the_scalar_path_and_still_matches(is_u8):
    u8, f32, perm = _sources(3, 8, 12)
    src = u8 if is_u8 else f32
    for pad in (65, 66, 67):
        assert torch.equal(_launch(src, perm, 1, 0.2871, None, pad=pad), _want(src, perm, 1, 0.2871, None))
        assert torch.equal(_launch(src, perm, 2, 0.5, (1, 7, 3, 10), pad=pad), _want(src, perm, 2, 0.5, (1, 7, 3, 10)))
    if not is_u8:                                     # an fp32 source that is only 4-byte aligned
        shifted = torch.empty(f32.numel() + 1, device='cuda')[1:].view_as(f32).copy_(f32)
        assert shifted.data_ptr() % 16 == 4
        assert torch.equal(_launch(shifted, perm, 1, 0.2871, None), _want(f32, perm, 1, 0.2871, None))
        assert torch.equal(_launch(shifted, perm, 2, 0.5, (1, 7, 3, 10)), _want(f32, perm, 2, 0.5, (1, 7, 3, 10)))


def test_apply_mix_is_apply_mix_torch_and_reads_nothing_back():
    from robustart_amd.train.mixing import apply_mix, apply_mix_torch, draw_mix
    u8, f32, _ = _sources(5, 6, 10)
    big, _, _ = _sources(2, 224, 224)
    plans = [draw_mix(0.2, None, 0, 3, 0, 5, 6, 10), draw_mix(None, 1.0, 0, 3, 0, 5, 6, 10)]
    for plan in plans:
        for src in (u8, f32):
            assert torch.equal(apply_mix(src, plan, 'cuda'), apply_mix_torch(src, plan))
    plan = draw_mix(None, 1.0, 0, 4, 0, 2, 224, 224)
    apply_mix(big, plan, 'cuda')                       # allocations warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = apply_mix(big, plan, 'cuda')
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(out, apply_mix_torch(big, plan))
    with pytest.raises(ValueError):
        apply_mix(u8, ('mixup', 0.5, np.array([0, 1, 2, 3, 5]), None), 'cuda')
    with pytest.raises(RuntimeError):
        apply_mix(u8.cpu(), plans[0], 'cpu')


# ---- rart_label_smooth_ce_mix_f32 ---------------------------------------------------------------------------------------------------------
def _ce_mix(z, ya, yb, s, lam, scale, want_loss=True, want_grad=True):
    from robustart_amd import _lib as L
    b, c = z.shape
    loss = torch.full((b,), float('nan'), device='cuda') if want_loss else None
    dl = torch.full_like(z, float('nan')) if want_grad else None
    L.check(L.load().rart_label_smooth_ce_mix_f32(z.data_ptr(), ya.data_ptr(), yb.data_ptr(), b, c, s, float(lam), scale, L.ptr(loss),
                                                  L.ptr(dl), L.stream_ptr()))
    return loss, dl


def _ce_inputs(b, c):
    g = torch.Generator().manual_seed(b * 7 + c)
    z = (torch.randn(b, c, generator=g) * 3.0).cuda()
    ya = torch.randint(0, c, (b,), generator=g)
    yb = torch.randint(0, c, (b,), generator=g)
    yb[::3] = ya[::3]                                  # rows whose two labels agree
    return z, ya.cuda(), yb.cuda()


@pytest.mark.parametrize('s', [0.0, 0.1])
@pytest.mark.parametrize('b,c', [(5, 1000), (3, 10), (70, 1000)])
def test_two_label_loss_against_the_one_label_entry(b, c, s):
    from robustart_amd.train.arena import label_smooth_ce
    z, ya, yb = _ce_inputs(b, c)
    assert bool((ya == yb).any()) and bool((ya != yb).any())
    scale = 1.0 / b
    la, da = label_smooth_ce(z, ya, s, scale)
    lb, db = label_smooth_ce(z, yb, s, scale)
    # lam = 1 / 0: the one-label entry on y_a / y_b, bit for bit
    l1, d1 = _ce_mix(z, ya, yb, s, 1.0, scale)
    assert torch.equal(l1, la) and torch.equal(d1, da)
    l0, d0 = _ce_mix(z, ya, yb, s, 0.0, scale)
    assert torch.equal(l0, lb) and torch.equal(d0, db)
    for lam in (0.5, 0.2871, float(np.random.default_rng(2).beta(0.2, 0.2))):
        loss, dl = _ce_mix(z, ya, yb, s, lam, scale)
        lam32, oml32 = torch.tensor(lam, dtype=torch.float32, device='cuda'), torch.tensor(1.0 - lam, dtype=torch.float32, device='cuda')
        prod_a, prod_b = lam32 * la, oml32 * lb                        # separate multiplies and a separate add: no contraction
        assert torch.equal(loss, prod_a + prod_b), lam
        # each side carries at most four roundings of terms of magnitude <= 1
        want = lam * da.double() + (1.0 - lam) * db.double()
        err = (dl.double() - want).abs().max().item()
        print('B %d C %d s %.1f lam %.4f: |dlogits - fp64 combination| max %.3e (bound %.3e)' % (b, c, s, lam, err, 8 * 2.0 ** -24 * scale))
        assert err <= 8 * 2.0 ** -24 * scale
        # fp64 autograd of the two-label loss on the same fp32 logits; the yardstick is the one-label entry's own error
        def autograd(loss_of):
            z64 = z.double().requires_grad_(True)
            rows = loss_of(z64)
            g, = torch.autograd.grad(rows.sum() * scale, z64)
            return rows.detach(), g
        ce = lambda zz, y: F.cross_entropy(zz, y, label_smoothing=s, reduction='none')      # noqa: E731
        ra, ga = autograd(lambda zz: ce(zz, ya))
        rb, gb = autograd(lambda zz: ce(zz, yb))
        rm, gm = autograd(lambda zz: lam * ce(zz, ya) + (1.0 - lam) * ce(zz, yb))
        base_l = max((la.double() - ra).abs().max().item(), (lb.double() - rb).abs().max().item())
        base_d = max((da.double() - ga).abs().max().item(), (db.double() - gb).abs().max().item())
        got_l, got_d = (loss.double() - rm).abs().max().item(), (dl.double() - gm).abs().max().item()
        print('   vs fp64 autograd: loss %.3e (one-label entry %.3e), dlogits %.3e (one-label entry %.3e)' % (got_l, base_l, got_d, base_d))
        assert got_d <= 2 * base_d
        # The twice-the-one-label-error bar is held by the gradient only.  The loss is pinned bit for bit above to the fp32 combination
        # lam32 * L_a + oml32 * L_b, and that fixed arithmetic cannot also stay within twice the one-label error: at 3 x 10, s = 0 the
        # one-label entry is 1.3e-7 from fp64 and the prescribed combination 3.0e-7 (2.2 x), since it adds the roundings of lam and
        # 1 - lam, of the two products and of the sum to the convex combination of the one-label errors.  So the loss is held to what
        # that arithmetic allows: the one-label error plus five half-ulps of a term no larger than the larger loss.
        assert got_l <= base_l + 3 * 2.0 ** -24 * max(la.max().item(), lb.max().item())
    # either output may be left out
    only_l, none = _ce_mix(z, ya, yb, s, 0.2871, scale, want_grad=False)
    none2, only_d = _ce_mix(z, ya, yb, s, 0.2871, scale, want_loss=False)
    both_l, both_d = _ce_mix(z, ya, yb, s, 0.2871, scale)
    assert none is None and none2 is None and torch.equal(only_l, both_l) and torch.equal(only_d, both_d)


def test_arena_wrapper_is_the_entry():
    from robustart_amd.train.arena import label_smooth_ce_mix
    z, ya, yb = _ce_inputs(5, 1000)
    loss, dl = label_smooth_ce_mix(z, ya, yb, 0.2871, 0.1, 0.2)
    l2, d2 = _ce_mix(z, ya, yb, 0.1, 0.2871, 0.2)
    assert torch.equal(loss, l2) and torch.equal(dl, d2)


# ---- one solver step per train engine -----------------------------------------------------------------------------------------------------
class _Args:
    engine = 'hip'
    train_engine = 'hip'
    corruption = None
    attack = None
    seed = 0
    max_iter = 2
    recover = None
    ckpt_dir = None


ENGINES = {
    # model block, (batch, input size), optimizer, (median, minimum) of the per-parameter gradient cosines of the engine's own test
    'resnet': ({'type': 'resnet50_official'}, (16, 64), {'type': 'SGD', 'kwargs': {'nesterov': True, 'momentum': 0.9, 'weight_decay': 1e-4}},
               (0.999, 0.99)),
    'vit': ({'type': 'vit_base', 'kwargs': {'depth': 2, 'drop_path_rate': 0.0}}, (4, 224), {'type': 'AdamW', 'kwargs': {'weight_decay': 0.05}},
            (0.999, 0.98)),
    'mixer': ({'type': 'mixer_b16_224', 'kwargs': {'depth': 2, 'drop_path_rate': 0.0}}, (4, 224),
              {'type': 'AdamW', 'kwargs': {'weight_decay': 0.05}}, (0.999, 0.99)),
}


def _engine_class(name):
    if name == 'resnet':
        from robustart_amd.model.train_engine import ResNet50TrainEngine as E
    elif name == 'vit':
        from robustart_amd.model.vit_train_engine import ViTTrainEngine as E
    else:
        from robustart_amd.model.mixer_train_engine import MixerTrainEngine as E
    return E


def _solver_cfg(name, keys, save_dir, **saver):
    model, (bs, size), opt, _ = ENGINES[name]
    lr = {'base_lr': 0.01, 'warmup_lr': 0.02} if opt['type'] == 'SGD' else {'base_lr': 1e-5, 'warmup_lr': 1e-3}
    cfg = {'model': model, 'optimizer': opt, 'lr_scheduler': {'kwargs': dict(lr, min_lr=0.0, warmup_steps=1)}, 'label_smooth': 0.1,
           'max_iter': 2, 'data': {'read_from': 'fake', 'fake_size': 2 * bs, 'batch_size': bs, 'input_size': size, 'seed': 11},
           'saver': dict(save_dir=save_dir, print_freq=100, **saver)}
    cfg.update(keys)
    return cfg


@pytest.mark.parametrize('keys', [{'mixup': 0.2}, {'cutmix': 1.0}], ids=['mixup', 'cutmix'])
@pytest.mark.parametrize('name', ['resnet', 'vit', 'mixer'])
def test_one_solver_step_on_a_mixed_batch(name, keys, tmp_path, monkeypatch):
    from robustart_amd.model import get_model
    from robustart_amd.train import cls_solver as S
    from robustart_amd.train.arena import label_smooth_ce
    from robustart_amd.train.mixing import apply_mix_torch, draw_mix, mix_alphas
    E = _engine_class(name)
    fwd, bwd = E.forward, E.backward
    cap = {}

    def spy_forward(self, src, *a, **k):
        out = fwd(self, src, *a, **k)
        if 'x' not in cap:
            cap['x'], cap['logits'], cap['engine'] = src.clone(), out.clone(), self
        return out

    def spy_backward(self, dlogits, *a, **k):
        r = bwd(self, dlogits, *a, **k)
        if 'grads' not in cap:
            cap['dlogits'] = dlogits.clone()
            cap['grads'] = [p.grad.clone() for p in self.model.parameters()]
        return r
    monkeypatch.setattr(E, 'forward', spy_forward)
    monkeypatch.setattr(E, 'backward', spy_backward)
    rank, world, device = S.init_dist()
    # the uninterrupted run: two iterations, a checkpoint after the first
    torch.manual_seed(5)
    cfg = _solver_cfg(name, keys, str(tmp_path / 'full'), val_freq=1, save_many=True)
    loss, m_full = S.train(cfg, _Args(), rank, world, device)
    assert np.isfinite(loss) and loss > 0 and 'grads' in cap
    monkeypatch.setattr(E, 'forward', fwd)
    monkeypatch.setattr(E, 'backward', bwd)

    # iteration 0 by hand: the same engine class on the same initial weights, apply_mix_torch, two calls of the one-label entry
    model_cfg, (bs, size), _, (bar_median, bar_min) = ENGINES[name]
    torch.manual_seed(5)
    model = get_model(model_cfg).to(device).train()
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    eng = E(model, device)
    d = cfg['data']
    sel, _ = S.EpochSampler(d['fake_size'], bs, 0, 1, d['seed'], True).batch(0)
    imgs, y = S.FakeImageNet(d['fake_size'], size).batch(sel, device)
    plan = draw_mix(*mix_alphas(cfg), d['seed'], 0, 0, bs, size, size)
    kind, lam, perm, box = plan
    assert kind == list(keys)[0]
    x_ref = apply_mix_torch(imgs, plan).contiguous()
    assert torch.equal(cap['x'], x_ref)                                  # the solver's launch formed the torch expression's batch
    logits = eng.forward(x_ref, False, S.IMAGENET_MEAN, S.IMAGENET_STD)
    assert torch.equal(cap['logits'], logits)
    yb = y[torch.from_numpy(perm).to(device)]
    _, da = label_smooth_ce(logits, y, 0.1, 1.0 / bs)
    _, db = label_smooth_ce(logits, yb, 0.1, 1.0 / bs)
    dl = lam * da + (1.0 - lam) * db
    assert (cap['dlogits'] - dl).abs().max().item() <= 8 * 2.0 ** -24 / bs
    eng.backward(dl)
    rep = []
    for (n, p), q in zip(model.named_parameters(), cap['grads']):
        if name == 'mixer' and n.endswith('.mlp_tokens.fc2.bias'):       # an exact gradient zero: rounding residue on both sides
            continue                                                     # (tests/test_mixer_train_gpu.py)
        a, b2 = q.double().flatten(), p.grad.double().flatten()
        rep.append((float((a @ b2) / (a.norm() * b2.norm() + 1e-300)), n))
    rep.sort()
    cs = np.array([c for c, _ in rep])
    print('%s %s lam %.4f: gradient cosine solver step vs by hand: median %.7f min %.7f (%s)' % (name, kind, lam, np.median(cs), cs.min(),
                                                                                                 rep[0][1]))
    assert np.median(cs) > bar_median and cs.min() > bar_min, rep[:6]

    # resumed after one iteration: the second iteration's draws and parameters are the uninterrupted run's, bit for bit
    a = _Args()
    a.recover = os.path.join(str(tmp_path / 'full'), 'ckpt_1.pth.tar')
    torch.manual_seed(99)
    _, m_res = S.train(_solver_cfg(name, keys, str(tmp_path / 'res')), a, rank, world, device)
    assert S.train.start_iter == 1
    for (k, v), (_, w) in zip(m_full.state_dict().items(), m_res.state_dict().items()):
        assert torch.equal(v, w), k
