"""Mixup / CutMix in the solver (`mixup`, `cutmix`; robustart_amd/train/mixing.py) without a GPU: the two library entries are declared,
exported and bound and check their arguments before any launch; the draws are a pure function of (seed, iteration, rank); the keys are
read as the reference's configs mean them; and the solver's CPU scaffold trains on the mixed batch with the two-label loss."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['rart_mix_batch_f32', 'rart_label_smooth_ce_mix_f32']


def test_new_symbols_are_declared_exported_and_bound():
    from robustart_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'robustart_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(rart_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for s in NEW:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.rart_version() == 110 == _lib.ABI_VERSION


def test_argument_checks_of_the_mix_entries_without_gpu():
    """every check happens before a launch; the pointers are never dereferenced"""
    from robustart_amd import _lib
    lib = _lib.load()
    p, q = 4096, 1 << 40
    mix = lambda *a: lib.rart_mix_batch_f32(*a, None)           # noqa: E731
    # the box must satisfy 0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w
    for box in ((0, 9, 0, 4), (0, 4, 0, 13), (-1, 4, 0, 4), (0, 4, -1, 4), (5, 4, 0, 4), (0, 4, 7, 6)):
        assert mix(p, 1, p, q, 2, 8, 12, 2, 0.5, *box) == 1, box
        assert b'box' in lib.rart_last_error_string()
    for mode in (0, 3):
        assert mix(p, 1, p, q, 2, 8, 12, mode, 0.5, 0, 4, 0, 4) == 1 and b'mode' in lib.rart_last_error_string()
    for lam in (-0.01, 1.01, float('nan')):
        assert mix(p, 0, p, q, 2, 8, 12, 1, lam, 0, 0, 0, 0) == 1 and b'lam' in lib.rart_last_error_string()
    for src, perm, dst in ((None, p, q), (p, None, q), (p, p, None)):
        assert mix(src, 1, perm, dst, 2, 8, 12, 1, 0.5, 0, 0, 0, 0) == 1 and b'null' in lib.rart_last_error_string()
    for n, h, w in ((0, 8, 12), (2, 0, 12), (2, 8, -4)):
        assert mix(p, 1, p, q, n, h, w, 1, 0.5, 0, 0, 0, 0) == 1
    # dst aliasing src: the same pointer, and a dst that starts inside src (fp32: 2 * 3 * 8 * 12 * 4 = 2304 bytes; u8: 576) or ends in it
    assert mix(q, 0, p, q, 2, 8, 12, 1, 0.5, 0, 0, 0, 0) == 1 and b'overlap' in lib.rart_last_error_string()
    assert mix(q, 1, p, q, 2, 8, 12, 2, 0.5, 0, 4, 0, 4) == 1
    assert mix(q, 0, p, q + 2300, 2, 8, 12, 1, 0.5, 0, 0, 0, 0) == 1
    assert mix(q, 1, p, q + 572, 2, 8, 12, 1, 0.5, 0, 0, 0, 0) == 1
    assert mix(q + 2300, 1, p, q, 2, 8, 12, 1, 0.5, 0, 0, 0, 0) == 1
    # 2^32 elements or more are refused (29000 x 3 x 224 x 224 = 4.4e9)
    assert mix(p, 1, p, q, 29000, 224, 224, 1, 0.5, 0, 0, 0, 0) == 1 and b'too many' in lib.rart_last_error_string()

    ce = lambda *a: lib.rart_label_smooth_ce_mix_f32(*a, None)  # noqa: E731
    for lam in (-0.01, 1.01, float('nan')):
        assert ce(p, p, p, 4, 10, 0.1, lam, 1.0, p, p) == 1 and b'lam' in lib.rart_last_error_string()
    assert ce(p, p, None, 4, 10, 0.1, 0.5, 1.0, p, p) == 1                  # null labels_b
    assert ce(p, None, p, 4, 10, 0.1, 0.5, 1.0, p, p) == 1 and ce(None, p, p, 4, 10, 0.1, 0.5, 1.0, p, p) == 1
    assert ce(p, p, p, 0, 10, 0.1, 0.5, 1.0, p, p) == 1 and ce(p, p, p, 4, 0, 0.1, 0.5, 1.0, p, p) == 1
    assert ce(p, p, p, 4, 10, 1.5, 0.5, 1.0, p, p) == 1 and b'label_smoothing' in lib.rart_last_error_string()
    assert ce(p, p, p, 4, 10, 0.1, 0.5, 1.0, None, None) == 1 and b'nothing to compute' in lib.rart_last_error_string()


# ---- draws ------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]


@pytest.mark.parametrize('alphas', [(0.2, None), (None, 1.0), (0.2, 1.0)])
def test_draw_mix_is_a_pure_function_of_its_key(alphas):
    from robustart_amd.train.mixing import draw_mix
    a = draw_mix(*alphas, 3, 7, 1, 16, 24, 40)
    np.random.seed(5)                                       # global generator state plays no part
    draw_mix(*alphas, 3, 8, 1, 16, 24, 40)                   # nor do earlier calls
    b = draw_mix(*alphas, 3, 7, 1, 16, 24, 40)
    assert _same(a, b)
    for other in ((3, 8, 1), (3, 7, 0), (4, 7, 1)):          # another iteration, rank, seed: another plan
        assert not _same(a, draw_mix(*alphas, *other, 16, 24, 40))
    assert draw_mix(None, None, 3, 7, 1, 16, 24, 40) is None


def test_plans_are_permutations_boxes_inside_and_exact_area_ratios():
    from robustart_amd.train.mixing import draw_mix
    for it in range(100):
        for B, H, W in ((5, 6, 10), (32, 224, 224), (1, 7, 3)):
            kind, lam, perm, box = draw_mix(0.2, None, 0, it, 0, B, H, W)
            assert kind == 'mixup' and box is None and 0.0 <= lam <= 1.0 and isinstance(lam, float)
            assert sorted(perm.tolist()) == list(range(B))
            kind, lam, perm, box = draw_mix(None, 1.0, 0, it, 0, B, H, W)
            y0, y1, x0, x1 = box
            assert kind == 'cutmix' and sorted(perm.tolist()) == list(range(B))
            assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
            assert lam == 1.0 - (y1 - y0) * (x1 - x0) / float(H * W)


def test_cutmix_box_at_the_ends_of_lam0():
    from robustart_amd.train.mixing import cutmix_box
    for cy, cx in ((0, 0), (11, 20), (23, 39)):
        assert cutmix_box(1.0, cy, cx, 24, 40) == ((cy, cy, cx, cx), 1.0)               # empty box: the own image, own label
    assert cutmix_box(0.0, 12, 20, 24, 40) == ((0, 24, 0, 40), 0.0)                     # the whole partner image
    box, lam = cutmix_box(0.0, 0, 0, 24, 40)                                            # a corner centre keeps a quarter
    assert box == (0, 12, 0, 20) and lam == 0.75
    box, lam = cutmix_box(0.5, 5, 7, 24, 40)                                            # r = sqrt(0.5): 16 x 28 around (5, 7), clipped
    assert box == (0, 13, 0, 21) and lam == 1.0 - 13 * 21 / 960.0


def test_both_keys_apply_exactly_one_operation_per_iteration():
    from robustart_amd.train.mixing import draw_mix
    kinds = []
    for it in range(200):
        kind, lam, perm, box = draw_mix(0.2, 1.0, 0, it, 0, 8, 32, 32)
        assert (kind == 'mixup' and box is None) or (kind == 'cutmix' and box is not None)
        kinds.append(kind)
    assert 60 <= kinds.count('mixup') <= 140 and kinds.count('mixup') + kinds.count('cutmix') == 200      # p = 1/2: 100 +- 5.7 sigma


def test_key_reading():
    from robustart_amd.train.mixing import mix_alphas
    assert mix_alphas({}) == (None, None)
    assert mix_alphas({'mixup': None, 'cutmix': None}) == (None, None)
    assert mix_alphas({'mixup': 1.0, 'cutmix': 0.0}) == (None, None)          # the reference's defaults: off
    assert mix_alphas({'mixup': 0.0}) == (None, None) and mix_alphas({'mixup': 1.5}) == (None, None)
    assert mix_alphas({'mixup': 0.2, 'cutmix': 1.0}) == (0.2, 1.0)            # augmentation/resnet50/config.yaml
    assert mix_alphas({'mixup': 0.2}) == (0.2, None) and mix_alphas({'cutmix': 1.0, 'mixup': 1.0}) == (None, 1.0)


def test_apply_mix_torch_on_u8_and_fp32_sources():
    from robustart_amd.train.mixing import apply_mix_torch
    u8 = torch.randint(0, 256, (3, 8, 12, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    x = u8.permute(0, 3, 1, 2).float().div(255.0)
    perm = np.array([0, 2, 1])
    for src in (u8, x.contiguous()):
        got = apply_mix_torch(src, ('mixup', 0.3, perm, None))
        assert torch.equal(got, 0.3 * x + (1.0 - 0.3) * x[[0, 2, 1]])
        got = apply_mix_torch(src, ('cutmix', 0.5, perm, (2, 6, 3, 9)))
        assert torch.equal(got[:, :, 2:6, 3:9], x[[0, 2, 1]][:, :, 2:6, 3:9])
        want = x.clone()
        want[:, :, 2:6, 3:9] = 0
        got[:, :, 2:6, 3:9] = 0
        assert torch.equal(got, want)
        assert torch.equal(apply_mix_torch(src, ('cutmix', 1.0, perm, (4, 4, 5, 5))), x)
    with pytest.raises(ValueError):
        apply_mix_torch(u8, ('mixup', 0.3, np.array([0, 3, 1]), None))


# ---- the solver's CPU scaffold ------------------------------------------------------------------------------------------------------------
def _tiny(**kw):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, stride=4), torch.nn.ReLU(), torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(),
                               torch.nn.Linear(4, 1000))


class _Args:
    engine, train_engine, max_iter = 'torch', 'hip', 2


def _cfg(**extra):
    cfg = {'model': {'type': 'tiny_test'}, 'data': {'fake_size': 22, 'batch_size': 4, 'input_size': 32, 'seed': 3},
           'label_smooth': 0.1, 'max_iter': 2, 'bf16': False, 'saver': {'print_freq': 1},
           'lr_scheduler': {'kwargs': {'base_lr': 0.01, 'warmup_lr': 0.02}}}
    cfg.update(extra)
    return cfg


def _solver_losses(cfg, monkeypatch, capsys):
    import robustart_amd.model as M
    from robustart_amd.train import cls_solver as S
    monkeypatch.setitem(M._REGISTRY, 'tiny_test', _tiny)
    capsys.readouterr()
    S.train(cfg, _Args(), 0, 1, torch.device('cpu'))
    return [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')]


def _by_hand(cfg, iters=2):
    """The scaffold's iterations restated: the sampler's batches, draw_mix's plans, the torch expressions for the images and
    lam * CE(a) + (1 - lam) * CE(b), torch.optim.SGD with the solver's default hyper-parameters."""
    from robustart_amd.train import cls_solver as S
    from robustart_amd.train.mixing import draw_mix, mix_alphas
    d = cfg['data']
    model = _tiny()
    opt = torch.optim.SGD(model.parameters(), lr=0.01, nesterov=True, momentum=0.9, weight_decay=1e-4)
    ds = S.FakeImageNet(d['fake_size'], d['input_size'])
    sampler = S.EpochSampler(d['fake_size'], d['batch_size'], 0, 1, d['seed'], True)
    mean, std = torch.tensor(S.IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(S.IMAGENET_STD).view(1, 3, 1, 1)
    lk = cfg['lr_scheduler']['kwargs']
    warm = S.resolve_schedule(cfg, d['fake_size'], d['batch_size'], 1)[1]
    mixup, cutmix = mix_alphas(cfg)
    out = []
    for it in range(iters):
        sel, _ = sampler.batch(it)
        imgs, y = ds.batch(sel, 'cpu')
        x = imgs.permute(0, 3, 1, 2).float().div(255.0)
        plan = draw_mix(mixup, cutmix, d['seed'], it, 0, len(sel), d['input_size'], d['input_size'])
        if plan is not None:
            kind, lam, perm, box = plan
            idx = torch.from_numpy(perm)
            if kind == 'mixup':
                x = lam * x + (1.0 - lam) * x[idx]
            else:
                y0, y1, x0, x1 = box
                x = x.clone()
                x[:, :, y0:y1, x0:x1] = x[idx][:, :, y0:y1, x0:x1]
        logits = model(((x - mean) / std).contiguous(memory_format=torch.channels_last)).float()
        if plan is None:
            loss = F.cross_entropy(logits, y, label_smoothing=0.1)
        else:
            loss = lam * F.cross_entropy(logits, y, label_smoothing=0.1) + (1.0 - lam) * F.cross_entropy(logits, y[idx], label_smoothing=0.1)
        opt.zero_grad()
        loss.backward()
        for g in opt.param_groups:
            g['lr'] = S.cosine_lr(it, iters, lk['base_lr'], lk['warmup_lr'], warm, 0.0)
        opt.step()
        out.append((float(loss.detach()), plan))
    return out


@pytest.mark.parametrize('keys', [{'mixup': 0.2}, {'cutmix': 1.0}])
def test_solver_scaffold_trains_on_the_mixed_batch_with_the_two_label_loss(keys, monkeypatch, capsys):
    """Two iterations reproduce the hand restatement to fp32 equality of the printed loss.  (`mixup: 0.2` is the case that fails on a
    solver that ignores the key.)"""
    cfg = _cfg(**keys)
    recs = _solver_losses(cfg, monkeypatch, capsys)
    want = _by_hand(cfg)
    assert [r['iter'] for r in recs] == [0, 1]
    for r, (loss, plan) in zip(recs, want):
        assert r['loss'] == loss
        assert r['mix'] == {'kind': plan[0], 'lam': plan[1]}
    # and the mixed run is not the plain run: the key is not ignored
    assert [w[0] for w in want] != [w[0] for w in _by_hand(_cfg())]


@pytest.mark.parametrize('keys', [{}, {'mixup': 1.0, 'cutmix': 0.0}])
def test_solver_scaffold_without_active_keys_is_the_plain_run(keys, monkeypatch, capsys):
    recs = _solver_losses(_cfg(**keys), monkeypatch, capsys)
    want = _by_hand(_cfg())
    assert [r['loss'] for r in recs] == [w[0] for w in want]
    assert all('mix' not in r for r in recs)


@pytest.mark.parametrize('keys', [{'mixup': 0.2}, {'cutmix': 1.0}, {'mixup': 0.2, 'cutmix': 1.0}])
def test_adv_train_with_an_active_mix_key_is_refused_before_the_device(keys, monkeypatch):
    import robustart_amd.model as M
    from robustart_amd.train import cls_solver as S
    monkeypatch.setitem(M._REGISTRY, 'tiny_test', _tiny)

    def no_device(self, *a, **k):
        raise AssertionError('the model was moved to a device')
    monkeypatch.setattr(torch.nn.Module, 'to', no_device)
    cfg = _cfg(adv_train={'eps': '4/255', 'steps': 1}, **keys)
    with pytest.raises(ValueError, match='adv_train together with an active'):
        S.train(cfg, _Args(), 0, 1, torch.device('cpu'))
    # inactive keys do not trigger the refusal: the run gets as far as moving the model
    with pytest.raises(AssertionError, match='moved to a device'):
        S.train(_cfg(adv_train={'eps': '4/255', 'steps': 1}, mixup=1.0, cutmix=0.0), _Args(), 0, 1, torch.device('cpu'))
