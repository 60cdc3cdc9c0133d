"""ConvNeXt-V2-B training on the MI355X: rart_cnx_grn_bwd_reduce_train_bf16 (csrc/convnext_v2.hip) against fp64 of the same bf16 operands
at the four stage shapes, ConvNeXtTrainEngine's V2 blocks against torch autograd through the fp32 ConvNeXtV2 module, one HIP AdamW step
against torch.optim.AdamW, the adversarial training loop of cls_solver (the pgd_adv_train/convnextv2 settings) including a
bit-identical resume, and a train step under torch.cuda.set_sync_debug_mode('error').

Bars: the kernel's fp32 outputs within 1e-5 relative + 1e-5 of the scale (the GRN statistics' tolerance, tests/test_convnext_v2_gpu.py);
the engine holds tests/test_convnext_train_gpu.py's bars for ConvNeXt-B."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EPS = 1e-6
HIDDEN = [(56 * 56, 512), (28 * 28, 1024), (14 * 14, 2048), (7 * 7, 4096), (77, 40)]     # (pixels, 4C): the stages at 224, one odd


def _lib():
    from robustart_amd import _lib as L
    return L, L.load()


def _close(got, ref, what):
    scale = ref.abs().max().item()
    err = (got.double() - ref).abs()
    bad = (err > 1e-5 * ref.abs() + 1e-5 * scale).sum().item()
    print('%s: max |err| %.3e (scale %.3e), %d outside' % (what, err.max().item(), scale, bad))
    assert bad == 0, what


def _train_reduce(g, y, G, w, B, P, C, acc=None):
    L, lib = _lib()
    need = lib.rart_cnx_grn_param_grad_workspace_bytes(B, C)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    a = torch.full((B, C), float('nan'), device='cuda')
    dw = acc[0] if acc is not None else torch.full((C,), float('nan'), device='cuda')
    db = acc[1] if acc is not None else torch.full((C,), float('nan'), device='cuda')
    L.check(lib.rart_cnx_grn_bwd_reduce_train_bf16(L.ptr(g), L.ptr(y), L.ptr(G), L.ptr(w), L.ptr(a), L.ptr(dw), L.ptr(db), B, P, C, EPS,
                                                   int(acc is not None), L.ptr(ws), need, L.stream_ptr()))
    return a, dw, db


@pytest.mark.parametrize('w_kind', ['random', 'zero'])
@pytest.mark.parametrize('shape', HIDDEN)
def test_grn_param_grad_kernel_vs_fp64(shape, w_kind):
    L, lib = _lib()
    P, C = shape
    B = 3
    gen = torch.Generator(device='cuda').manual_seed(P + C + (w_kind == 'zero'))
    y = F.gelu(torch.randn(B, P, C, device='cuda', generator=gen))
    y[1, :, 5] = 0.0                                                   # one all-zero channel: G == 0
    y = y.to(torch.bfloat16).contiguous()
    g = torch.randn(B, P, C, device='cuda', generator=gen).to(torch.bfloat16).contiguous()
    w = (0.5 * torch.randn(C, device='cuda', generator=gen)) if w_kind == 'random' else torch.zeros(C, device='cuda')
    sp = L.stream_ptr()
    G = torch.empty(B, C, device='cuda')
    L.check(lib.rart_cnx_grn_stats_bf16(L.ptr(y), L.ptr(G), B, P, C, sp))
    a, dw, db = _train_reduce(g, y, G, w, B, P, C)
    assert torch.isfinite(a).all() and torch.isfinite(dw).all() and torch.isfinite(db).all()
    # fp64 of the same bf16 operands
    yv, gv = y.double(), g.double()
    Gr = torch.sqrt((yv * yv).sum(1))
    N = Gr / (Gr.mean(1, keepdim=True) + EPS)
    tag = '%s w %s' % (shape, w_kind)
    _close(dw, (N * (gv * yv).sum(1)).sum(0), 'GRN dw ' + tag)
    _close(db, gv.sum((0, 1)), 'GRN db ' + tag)
    # a: the bits of rart_cnx_grn_bwd_reduce_bf16, which rart_cnx_grn_bwd_apply_bf16 consumes
    a0 = torch.empty(B, C, device='cuda')
    L.check(lib.rart_cnx_grn_bwd_reduce_bf16(L.ptr(g), L.ptr(y), L.ptr(w), L.ptr(a0), B, P, C, sp))
    assert torch.equal(a, a0)
    # repeat: bit-identical; one image alone: its `a` unchanged; accumulate adds
    a2, dw2, db2 = _train_reduce(g, y, G, w, B, P, C)
    assert torch.equal(a, a2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    a1, _, _ = _train_reduce(g[2:].contiguous(), y[2:].contiguous(), G[2:].contiguous(), w, 1, P, C)
    assert torch.equal(a1[0], a[2])
    pre_w, pre_b = torch.randn(C, device='cuda'), torch.randn(C, device='cuda')
    _, aw, ab = _train_reduce(g, y, G, w, B, P, C, acc=(pre_w.clone(), pre_b.clone()))
    assert torch.equal(aw, pre_w + dw) and torch.equal(ab, pre_b + db)


def _model(depths, grn_kind, seed=3):
    from robustart_amd.model.convnext_torch import ConvNeXtV2
    torch.manual_seed(seed)
    m = ConvNeXtV2(depths=depths, num_classes=1000).cuda().train()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if '.grn.' in n:
                p.copy_((0.5 * torch.randn(p.shape, generator=g)).cuda() if grn_kind == 'random' else torch.zeros_like(p))
            elif n.endswith('bias'):
                p.copy_((torch.randn(p.shape, generator=g) * 0.05).cuda())
            elif p.dim() == 1:                                             # LayerNorm weights
                p.copy_((1 + torch.randn(p.shape, generator=g) * 0.1).cuda())
    return m


def _engine_vs_autograd(depths, side, B, grn_kind):
    from robustart_amd.model.convnext_train_engine import ConvNeXtTrainEngine
    from robustart_amd.train.arena import label_smooth_ce
    model = _model(depths, grn_kind)
    ref = copy.deepcopy(model)
    for p in model.parameters():
        p.grad = torch.full_like(p, float('nan'))
    ready = []
    eng = ConvNeXtTrainEngine(model, 'cuda', on_grad_ready=lambda p: ready.append(id(p)))
    assert eng.grn
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
    grn = [r for r in rep if '.grn.' in r[2]]
    assert len(grn) == 2 * sum(depths)
    rep.sort()
    cs = np.array([c for c, _, _ in rep])
    print('V2 depths %s %dx%d B=%d grn %s: logits cos %.7f, |dloss| %.2e; gradient cos median %.6f; lowest %s; GRN lowest %s'
          % (depths, side, side, B, grn_kind, cos, dloss, np.median(cs), [(round(c, 5), round(r, 4), n) for c, r, n in rep[:4]],
             [(round(c, 5), round(r, 4), n) for c, r, n in sorted(grn)[:2]]))
    assert cos > 0.99997 and dloss < 1e-3 * loss.item()
    assert np.median(cs) > 0.999 and cs.min() > 0.99, rep[:8]
    assert all(0.97 < r < 1.03 for _, r, _ in rep), [x for x in rep if not 0.97 < x[1] < 1.03][:8]
    # backward again from the same forward: bit-identical gradients, every parameter announced once more
    ready.clear()
    eng.backward(dl)
    assert len(ready) == len(grads) and len(set(ready)) == len(grads)
    for p, q in zip(model.parameters(), grads):
        assert torch.equal(p.grad, q)


@pytest.mark.parametrize('grn_kind', ['random', 'zero'])
def test_v2_train_engine_reduced_depth_matches_torch_autograd(grn_kind):
    _engine_vs_autograd((1, 1, 2, 1), 96, 4, grn_kind)


@pytest.mark.parametrize('grn_kind', ['random', 'zero'])
def test_v2_train_engine_convnextv2_base_matches_torch_autograd(grn_kind):
    _engine_vs_autograd((3, 3, 27, 3), 224, 2, grn_kind)


def test_v2_one_hip_adamw_step_matches_torch_adamw_and_repack_follows():
    from robustart_amd.model.convnext_train_engine import ConvNeXtTrainEngine
    from robustart_amd.train.arena import HipOptimizer, ParamArena, label_smooth_ce
    model = _model((1, 1, 2, 1), 'zero', seed=7)
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
    print('V2 AdamW step: update cosine %.5f, worst parameter difference %.2e (lr 1e-3)' % (cos, worst))
    assert cos > 0.99 and worst <= 2.0e-3 + 1e-6
    # GRN left timm's zero init, and the repacked tables carry the updated values
    grn = [(n, p) for n, p in model.named_parameters() if '.grn.' in n]
    assert all(p.detach().abs().max().item() > 0 for _, p in grn)
    eng.repack()
    tab = [t for S in eng.stages for L in S['blocks'] for t in (L['grn_w'], L['grn_b'])]
    assert len(tab) == len(grn) and all(torch.equal(t, p.detach()) for t, (_, p) in zip(tab, grn))
    out = eng.forward(x01, False, MEAN, STD)
    assert torch.isfinite(out).all()
    fresh = ConvNeXtTrainEngine(model, 'cuda').forward(x01, False, MEAN, STD)
    assert torch.equal(out, fresh)                                          # nothing in the tables is stale
    assert not torch.equal(out, logits)


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
    """exprs/nips_benchmark/pgd_adv_train/convnextv2/config.yaml (AdamW wd 0.05, no_wd fc / norm False, label smoothing 0.1, EMA
    0.9999, drop_path_rate 0.0) on fake data, plus a 2-step PGD inner loop"""
    return {'model': {'type': 'convnextv2_base', 'kwargs': {'num_classes': 1000, 'drop_path_rate': 0.0}},
            'optimizer': {'type': 'AdamW', 'no_wd': {'fc': False, 'norm': False}, 'kwargs': {'weight_decay': 0.05}},
            'lr_scheduler': {'kwargs': {'base_lr': 0.00001, 'warmup_lr': 0.0005, 'min_lr': 0.00001, 'warmup_steps': 1}},
            'label_smooth': 0.1, 'ema': {'enable': True, 'kwargs': {'decay': 0.9999}}, 'max_iter': 2,
            'adv_train': {'eps': '4/255', 'steps': 2},
            'data': {'read_from': 'fake', 'fake_size': 8, 'batch_size': 4, 'input_size': 64},
            'saver': dict(save_dir=save_dir, print_freq=100, **saver)}


def test_cls_solver_adversarially_trains_convnextv2_base(tmp_path, monkeypatch):
    from robustart_amd.model.convnext_train_engine import ConvNeXtTrainEngine
    from robustart_amd.model.engine import EngineModel
    from robustart_amd.train import cls_solver as S
    built, refolds = [], []
    init, refold = ConvNeXtTrainEngine.__init__, EngineModel.rart_refold

    def spy_init(self, model, *a, **k):
        built.append(bool(getattr(model, 'use_grn', False)))
        init(self, model, *a, **k)

    def spy_refold(self, torch_model=None):
        refold(self, torch_model)
        refolds.append(self.rart_engine.grn)
    monkeypatch.setattr(ConvNeXtTrainEngine, '__init__', spy_init)
    monkeypatch.setattr(EngineModel, 'rart_refold', spy_refold)
    rank, world, device = S.init_dist()
    torch.manual_seed(5)
    loss, m_full = S.train(_solver_cfg(str(tmp_path / 'full')), _Args(), rank, world, device)
    print('convnextv2_base adversarial training, 2 iterations: last loss %.4f' % loss)
    assert np.isfinite(loss) and loss > 0
    assert built == [True]                          # the V2 model trains on ConvNeXtTrainEngine
    assert refolds == [True]                        # the attack engine (V2) is refolded from the live weights at iteration 2
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
    assert any('.grn.' in k for k in ck_a['ema'])
    for k in ck_a['ema']:
        assert torch.equal(ck_a['ema'][k], ck_b['ema'][k]), k


def test_v2_train_step_makes_no_device_to_host_read():
    from robustart_amd.model.convnext_train_engine import ConvNeXtTrainEngine
    from robustart_amd.train.arena import label_smooth_ce
    model = _model((1, 1, 2, 1), 'random')
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
