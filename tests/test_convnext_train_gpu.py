"""ConvNeXt-B training on the MI355X: the depthwise weight-gradient and layer-scale kernels (csrc/convnext_train.hip) against fp64,
ConvNeXtTrainEngine against torch autograd through the fp32 module, one HIP AdamW step against torch.optim.AdamW, and the adversarial
training loop of cls_solver (the pgd_adv_train/convnext_base settings) including a bit-identical resume."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _lib():
    from robustart_amd import _lib as L
    return L, L.load()


def _dwconv_wgrad(x, dz, n, h, w, c, layout=0, acc=None):
    L, lib = _lib()
    need = lib.rart_cnx_dwconv_wgrad_workspace_bytes(n, h, w, c)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    dw = acc[0] if acc is not None else torch.full((49, c) if layout == 0 else (c, 49), float('nan'), device='cuda')
    db = acc[1] if acc is not None else torch.full((c,), float('nan'), device='cuda')
    L.check(lib.rart_cnx_dwconv_wgrad_bf16(L.ptr(x), L.ptr(dz), L.ptr(dw), L.ptr(db), n, h, w, c, layout, int(acc is not None),
                                           L.ptr(ws), need, L.stream_ptr()))
    return dw, db


@pytest.mark.parametrize('n,h,w,c', [(2, 56, 56, 128), (2, 28, 28, 256), (2, 14, 14, 512), (3, 7, 7, 1024),
                                     (1, 7, 9, 40), (2, 13, 17, 72), (1, 56, 56, 8)])
def test_dwconv_wgrad_matches_fp64_autograd(n, h, w, c):
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + c)
    x = torch.randn(n, h, w, c, generator=g).to(torch.bfloat16).cuda()
    dz = (torch.randn(n, h, w, c, generator=g) * 0.1).to(torch.bfloat16).cuda()
    dw, db = _dwconv_wgrad(x, dz, n, h, w, c)
    x64 = x.double().permute(0, 3, 1, 2)
    wt = torch.zeros(c, 1, 7, 7, dtype=torch.float64, device='cuda', requires_grad=True)
    bt = torch.zeros(c, dtype=torch.float64, device='cuda', requires_grad=True)
    F.conv2d(x64, wt, bt, padding=3, groups=c).backward(dz.double().permute(0, 3, 1, 2))
    ref_w, ref_b = wt.grad.reshape(c, 49).t(), bt.grad
    err_w = ((dw.double() - ref_w).norm(dim=0) / ref_w.norm(dim=0)).max().item()
    err_b = ((db.double() - ref_b).abs() / ref_b.abs().clamp_min(1e-3 * ref_b.abs().max())).max().item()
    print('dwconv wgrad %s: worst per-channel relative error dw %.2e, db %.2e' % ((n, h, w, c), err_w, err_b))
    assert err_w < 2e-5 and err_b < 1e-4
    dw2, db2 = _dwconv_wgrad(x, dz, n, h, w, c)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)                         # deterministic
    dwt, dbt = _dwconv_wgrad(x, dz, n, h, w, c, layout=1)
    assert torch.equal(dwt, dw.t()) and torch.equal(dbt, db)                     # the module layout [c][49]
    pre_w, pre_b = torch.randn(49, c, device='cuda'), torch.randn(c, device='cuda')
    aw, ab = _dwconv_wgrad(x, dz, n, h, w, c, acc=(pre_w.clone(), pre_b.clone()))
    assert torch.equal(aw, pre_w + dw) and torch.equal(ab, pre_b + db)          # accumulate adds


@pytest.mark.parametrize('gamma_kind', ['init', 'trained'])
@pytest.mark.parametrize('rows,c', [(2 * 3136, 128), (2 * 49, 1024), (77, 40)])
def test_layer_scale_fwd_bwd_match_fp64(rows, c, gamma_kind):
    L, lib = _lib()
    g = torch.Generator().manual_seed(rows + c)
    gamma = (torch.full((c,), 1e-6) if gamma_kind == 'init' else 0.2 + 0.6 * torch.rand(c, generator=g)).cuda()
    dx = torch.randn(rows, c, generator=g).to(torch.bfloat16).cuda()
    u2 = torch.randn(rows, c, generator=g).to(torch.bfloat16).cuda()
    x_in = torch.randn(rows, c, generator=g).to(torch.bfloat16).cuda()
    x_out = torch.empty_like(x_in)
    L.check(lib.rart_cnx_layer_scale_fwd_bf16(L.ptr(x_in), L.ptr(u2), L.ptr(gamma), L.ptr(x_out), rows, c, L.stream_ptr()))
    want = x_in.double() + gamma.double() * u2.double()
    assert ((x_out.double() - want).abs() <= want.abs() * 2.0 ** -8 + 1e-30).all()              # one bf16 rounding
    need = lib.rart_cnx_layer_scale_bwd_workspace_bytes(rows, c)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')

    def run(db_on=True):
        dv = torch.empty_like(dx)
        dg = torch.full((c,), float('nan'), device='cuda')
        db = torch.full((c,), float('nan'), device='cuda') if db_on else None
        L.check(lib.rart_cnx_layer_scale_bwd_bf16(L.ptr(dx), L.ptr(u2), L.ptr(gamma), L.ptr(dv), L.ptr(dg), L.ptr(db), rows, c, 0,
                                                  L.ptr(ws), need, L.stream_ptr()))
        return dv, dg, db
    dv, dg, db = run()
    ref_g = (dx.double() * u2.double()).sum(0)
    ref_b = (gamma.double() * dx.double()).sum(0)
    assert torch.equal(dv, (gamma * dx.float()).to(torch.bfloat16))
    scale_g, scale_b = ref_g.abs().max(), ref_b.abs().max()
    err_g = ((dg.double() - ref_g).abs() / scale_g).max().item()
    err_b = ((db.double() - ref_b).abs() / scale_b).max().item()
    print('layer scale %s gamma %s: dgamma %.2e, db2 %.2e of scale' % ((rows, c), gamma_kind, err_g, err_b))
    assert err_g < 1e-5 and err_b < 1e-5
    dv2, dg2, db2 = run()
    assert torch.equal(dv, dv2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    dv3, dg3, _ = run(db_on=False)
    assert torch.equal(dv, dv3) and torch.equal(dg, dg3)


def _model(depths, gamma_kind, seed=3):
    from robustart_amd.model.convnext_torch import ConvNeXt
    torch.manual_seed(seed)
    m = ConvNeXt(depths=depths, num_classes=1000).cuda().train()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias'):
                p.copy_((torch.randn(p.shape, generator=g) * 0.05).cuda())
            elif p.dim() == 1 and 'gamma' not in n:                              # LayerNorm weights
                p.copy_((1 + torch.randn(p.shape, generator=g) * 0.1).cuda())
            elif n.endswith('gamma') and gamma_kind == 'trained':
                p.copy_((0.2 + 0.6 * torch.rand(p.shape, generator=g)).cuda())
    return m


def _engine_vs_autograd(depths, side, B, gamma_kind):
    from robustart_amd.model.convnext_train_engine import ConvNeXtTrainEngine
    from robustart_amd.train.arena import label_smooth_ce
    model = _model(depths, gamma_kind)
    ref = copy.deepcopy(model)
    for p in model.parameters():
        p.grad = torch.full_like(p, float('nan'))
    ready = []
    eng = ConvNeXtTrainEngine(model, 'cuda', on_grad_ready=lambda p: ready.append(id(p)))
    x01 = torch.rand(B, 3, side, side, device='cuda')
    y = torch.randint(0, 1000, (B,), device='cuda')
    logits = eng.forward(x01, False, MEAN, STD)
    loss_rows, dl = label_smooth_ce(logits, y, 0.1, 1.0 / B)
    eng.backward(dl)
    assert len(ready) == len(set(ready)) and sorted(ready) == sorted(id(p) for p in model.parameters())
    grads = [p.grad.clone() for p in model.parameters()]
    mean = torch.tensor(MEAN, device='cuda').view(1, 3, 1, 1)
    std = torch.tensor(STD, device='cuda').view(1, 3, 1, 1)
    out = ref((x01 - mean) / std)
    loss = F.cross_entropy(out, y, label_smoothing=0.1)
    loss.backward()
    a, b = logits.double().flatten(), out.detach().double().flatten()
    cos = float((a @ b) / (a.norm() * b.norm()))
    dloss = abs(loss_rows.mean().item() - loss.item())
    rep = []
    for (n, p), q in zip(ref.named_parameters(), grads):
        ga, gb = q.double().flatten(), p.grad.double().flatten()
        rep.append((float((ga @ gb) / (ga.norm() * gb.norm() + 1e-300)), float(ga.norm() / (gb.norm() + 1e-300)), n))
    rep.sort()
    cs = np.array([c for c, _, _ in rep])
    print('depths %s %dx%d B=%d gamma %s: logits cos %.7f, |dloss| %.2e; gradient cos median %.6f; lowest %s'
          % (depths, side, side, B, gamma_kind, cos, dloss, np.median(cs), [(round(c, 5), round(r, 4), n) for c, r, n in rep[:4]]))
    # the bf16 forward's floor: the eval engine's logits carry the same ~7e-3-of-scale rounding (tests/test_convnext_gpu.py)
    assert cos > 0.99997 and dloss < 1e-3 * loss.item()
    assert np.median(cs) > 0.999 and cs.min() > 0.99, rep[:8]
    assert all(0.97 < r < 1.03 for _, r, _ in rep), [x for x in rep if not 0.97 < x[1] < 1.03][:8]
    # backward again from the same forward: bit-identical gradients, every parameter announced once more
    ready.clear()
    eng.backward(dl)
    assert len(ready) == len(grads)
    for p, q in zip(model.parameters(), grads):
        assert torch.equal(p.grad, q)


@pytest.mark.parametrize('gamma_kind', ['init', 'trained'])
def test_train_engine_reduced_depth_matches_torch_autograd(gamma_kind):
    _engine_vs_autograd((1, 1, 2, 1), 96, 4, gamma_kind)


@pytest.mark.parametrize('gamma_kind', ['init', 'trained'])
def test_train_engine_convnext_base_matches_torch_autograd(gamma_kind):
    _engine_vs_autograd((3, 3, 27, 3), 224, 2, gamma_kind)


def test_one_hip_adamw_step_matches_torch_adamw():
    from robustart_amd.model.convnext_train_engine import ConvNeXtTrainEngine
    from robustart_amd.train.arena import HipOptimizer, ParamArena, label_smooth_ce
    model = _model((1, 1, 2, 1), 'trained', seed=7)
    ref = copy.deepcopy(model)
    arena = ParamArena(model)
    opt = HipOptimizer(arena, kind='AdamW', lr=1e-3, weight_decay=0.05, betas=(0.9, 0.999), eps=1e-8)
    eng = ConvNeXtTrainEngine(model, 'cuda', on_grad_ready=arena.grad_ready)
    B = 4
    x01 = torch.rand(B, 3, 64, 64, device='cuda')
    y = torch.randint(0, 1000, (B,), device='cuda')
    logits = eng.forward(x01, False, MEAN, STD)
    _, dl = label_smooth_ce(logits, y, 0.1, 1.0 / B)
    eng.backward(dl)
    arena.finish_grad_exchange()
    opt.step(grad_scale=1.0)
    mean = torch.tensor(MEAN, device='cuda').view(1, 3, 1, 1)
    std = torch.tensor(STD, device='cuda').view(1, 3, 1, 1)
    before = [p.detach().clone() for p in ref.parameters()]
    F.cross_entropy(ref((x01 - mean) / std), y, label_smoothing=0.1).backward()
    topt = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=0.05, betas=(0.9, 0.999), eps=1e-8)
    topt.step()
    da = torch.cat([(p.detach() - b0).flatten() for p, b0 in zip(model.parameters(), before)]).double()
    db = torch.cat([(p.detach() - b0).flatten() for p, b0 in zip(ref.parameters(), before)]).double()
    cos = float((da @ db) / (da.norm() * db.norm()))
    worst = max((p.detach() - q.detach()).abs().max().item() for p, q in zip(model.parameters(), ref.parameters()))
    print('AdamW step: update cosine %.5f, worst parameter difference %.2e (lr 1e-3)' % (cos, worst))
    assert cos > 0.99 and worst <= 2.0e-3 + 1e-6
    eng.repack()                                                                # the tables follow the updated master weights
    assert torch.isfinite(eng.forward(x01, False, MEAN, STD)).all()


class _Args:
    engine = 'hip'
    train_engine = 'hip'
    corruption = None
    attack = None
    seed = 0
    max_iter = 2
    recover = None
    ckpt_dir = None


def _solver_cfg(save_dir=None, **saver):
    """exprs/nips_benchmark/pgd_adv_train/convnext_base/config.yaml (AdamW wd 0.05, no_wd fc / norm False, label smoothing 0.1, EMA
    0.9999, drop_path_rate 0.0) on fake data, plus a 2-step PGD inner loop"""
    return {'model': {'type': 'convnext_base', 'kwargs': {'num_classes': 1000, 'drop_path_rate': 0.0}},
            'optimizer': {'type': 'AdamW', 'no_wd': {'fc': False, 'norm': False}, 'kwargs': {'weight_decay': 0.05}},
            'lr_scheduler': {'kwargs': {'base_lr': 0.00001, 'warmup_lr': 0.0005, 'min_lr': 0.00001, 'warmup_steps': 1}},
            'label_smooth': 0.1, 'ema': {'enable': True, 'kwargs': {'decay': 0.9999}}, 'max_iter': 2,
            'adv_train': {'eps': '4/255', 'steps': 2},
            'data': {'read_from': 'fake', 'fake_size': 8, 'batch_size': 4, 'input_size': 64},
            'saver': dict(save_dir=save_dir, print_freq=100, **saver)}


def test_cls_solver_adversarially_trains_convnext_base(tmp_path):
    from robustart_amd.train import cls_solver as S
    rank, world, device = S.init_dist()
    torch.manual_seed(5)
    loss, m_full = S.train(_solver_cfg(str(tmp_path / 'full')), _Args(), rank, world, device)
    print('convnext_base adversarial training, 2 iterations: last loss %.4f' % loss)
    assert np.isfinite(loss) and loss > 0
    # resume after iteration 1 reproduces iteration 2 bit-identically
    torch.manual_seed(5)
    S.train(_solver_cfg(str(tmp_path / 'part'), val_freq=1, save_many=True), _Args(), rank, world, device)
    a = _Args()
    a.recover = os.path.join(str(tmp_path / 'part'), 'ckpt_1.pth.tar')
    torch.manual_seed(99)
    _, m_res = S.train(_solver_cfg(str(tmp_path / 'res')), a, rank, world, device)
    assert S.train.start_iter == 1
    for (k, v), (_, w) in zip(m_full.state_dict().items(), m_res.state_dict().items()):
        assert torch.equal(v, w), k
    ck_a = torch.load(os.path.join(str(tmp_path / 'full'), 'ckpt.pth.tar'), weights_only=True)
    ck_b = torch.load(os.path.join(str(tmp_path / 'res'), 'ckpt.pth.tar'), weights_only=True)
    for k in ck_a['ema']:
        assert torch.equal(ck_a['ema'][k], ck_b['ema'][k]), k


def test_train_step_makes_no_device_to_host_read():
    from robustart_amd.model.convnext_train_engine import ConvNeXtTrainEngine
    from robustart_amd.train.arena import label_smooth_ce
    model = _model((1, 1, 2, 1), 'trained')
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    eng = ConvNeXtTrainEngine(model, 'cuda')
    B = 2
    x01 = torch.rand(B, 3, 64, 64, device='cuda')
    y = torch.randint(0, 1000, (B,), device='cuda')
    eng.backward(label_smooth_ce(eng.forward(x01, False, MEAN, STD), y, 0.1, 1.0 / B)[1])        # allocations warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        logits = eng.forward(x01, False, MEAN, STD)
        eng.backward(label_smooth_ce(logits, y, 0.1, 1.0 / B)[1])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
