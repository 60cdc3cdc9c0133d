"""MLP-Mixer-B/16 training on the MI355X: rart_tokmix_wgrad_bf16 / rart_tok_rowsum_bf16 (csrc/mixer_train.hip) against fp64 of the same
bf16 operands, MixerTrainEngine against torch autograd through the fp32 MlpMixer module, one HIP AdamW step against torch.optim.AdamW,
the adversarial training loop of cls_solver (the pgd_adv_train/mixer_B16_224 settings) including a bit-identical resume, and a train
step under torch.cuda.set_sync_debug_mode('error').

Bars:
  * kernels: bf16 products are exact in fp32 and the accumulation is fp32 in some fixed order, so per element
    |got - ref| <= (B D + splits) 2^-24 sum_b sum_d |p| |q|   (row sums: (B D + chunks) 2^-24 sum |x|), the right-hand side in fp64;
    a second run is bit-identical and `accumulate` adds to a pre-filled gradient exactly;
  * engine: tests/test_convnext_train_gpu.py's bars for a bf16 train engine: logits cosine > 0.99997, |dloss| < 1e-3 loss,
    per-parameter gradient cosine median > 0.999 and minimum > 0.99, norm ratio in (0.97, 1.03).  The same quantities of torch's own
    bf16-autocast autograd against the fp32 run are printed next to them.
  * one parameter class cannot be held to the cosine / norm-ratio bars by any bf16 step: `mlp_tokens.fc2.bias`.  b2[t] shifts every
    channel of token t by the same amount and every reader of the residual stream is a LayerNorm over channels, which ignores such a
    shift, so the exact gradient is zero and the fp32 "reference" is its own rounding noise (the test prints its size next to the fc1 biases').
    Measured on the MI355X against the fp32 run: engine cosine -0.15 / -0.07 (depth 2, B = 4) and -0.16 at worst (B/16, B = 2), norm
    ratio up to 6 637 and 19 845; torch's bf16-autocast autograd of the same module: cosine 0.09 and -0.19 at worst, norm ratio up to
    8 086 and 21 188.  For this class the engine is held to torch's bf16 autocast instead: its L2 distance to the fp32 gradient, over
    the class, must not exceed autocast's.  Every other parameter holds the bars above."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_mixer_train_cpu import tok_param_grads_fp64

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
U32 = 2.0 ** -24
# (M, N, D, B, slack rows): the two tables of a B/16 block at three batches, and one odd shape with a D tail
CASES = [(384, 196, 768, B, 3) for B in (1, 3, 8)] + [(196, 384, 768, B, 3) for B in (1, 3, 8)] + [(40, 24, 72, 5, 2)]


def _lib():
    from robustart_amd import _lib as L
    return L, L.load()


def _slabs(B, rows, D, slack, gen, poison):
    """bf16 [B][rows + slack][D]: the first `rows` rows of every image random, the slack rows NaN / inf"""
    t = torch.full((B, rows + slack, D), poison, device='cuda')
    t[:, :rows] = torch.randn(B, rows, D, device='cuda', generator=gen)
    return t.to(torch.bfloat16).contiguous()


def _wgrad(p, q, M, N, D, B, splits, per, grad, accumulate=0):
    from robustart_amd.model.engine_base import tokmix_wgrad_desc
    L, lib = _lib()
    ld = (M + 7) // 8 * 8
    part = torch.full((splits * N * ld,), float('nan'), device='cuda')
    d = tokmix_wgrad_desc(p, q, part, M, N, D, B, splits, per, ld, p_stride=p.shape[1] * D, q_stride=q.shape[1] * D)
    L.check(lib.rart_tokmix_wgrad_bf16(ctypes.byref(d), L.stream_ptr()))
    L.check(lib.rart_wgrad_reduce_f32(L.ptr(part), splits, 1, N, N, M, ld, L.ptr(grad), accumulate, L.stream_ptr()))
    return grad


def _rowsum(x, M, D, B, out, accumulate=0):
    L, lib = _lib()
    need = lib.rart_tok_rowsum_workspace_bytes(M, B)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    L.check(lib.rart_tok_rowsum_bf16(L.ptr(x), M, D, B, x.shape[1] * D, L.ptr(out), accumulate, L.ptr(ws), need, L.stream_ptr()))
    return out, need // (4 * M)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'M%d-N%d-D%d-B%d' % c[:4])
def test_token_gradient_kernels_vs_fp64(case):
    from robustart_amd.model.engine_base import EngineBase, wgrad_split_tokens
    M, N, D, B, slack = case
    gen = torch.Generator(device='cuda').manual_seed(M + 3 * N + 5 * D + 7 * B)
    p = _slabs(B, M, D, slack, gen, float('nan'))
    q = _slabs(B, N, D, slack, gen, float('inf'))
    pv, qv = p[:, :M].double(), q[:, :N].double()
    ref = torch.einsum('bmd,bnd->mn', pv, qv)
    mag = torch.einsum('bmd,bnd->mn', pv.abs(), qv.abs())
    # the engine's split, every image its own split, an uneven split, and one whose last split holds no image
    rule = wgrad_split_tokens(B, M, N, EngineBase.wgrad_target_wgs)
    worst = 0.0
    for splits, per in sorted({rule, (B, 1), ((B + 2) // 3, 3), ((B + 2) // 3 + 1, 3), (1, B)}):
        g = _wgrad(p, q, M, N, D, B, splits, per, torch.full((M, N), float('nan'), device='cuda'))
        assert torch.isfinite(g).all(), (splits, per)
        ratio = ((g.double() - ref).abs() / ((B * D + splits) * U32 * mag)).max().item()
        worst = max(worst, ratio)
        g2 = _wgrad(p, q, M, N, D, B, splits, per, torch.full((M, N), float('nan'), device='cuda'))
        assert torch.equal(g, g2), 'second run differs (splits %d)' % splits
        pre = torch.randn(M, N, device='cuda', generator=gen)
        acc = _wgrad(p, q, M, N, D, B, splits, per, pre.clone(), accumulate=1)
        assert torch.equal(acc, pre + g), 'accumulate (splits %d)' % splits
    print('token wgrad %s: worst |err| / bound = %.4f (rule: %d splits x %d images)' % (case[:4], worst, rule[0], rule[1]))
    assert worst <= 1.0
    # the fp64 oracle of the CPU suite states the same product (P = du_tok, Q = ln1 -> dW1)
    dW1 = tok_param_grads_fp64(pv.cpu().numpy(), qv.cpu().numpy(), qv.cpu().numpy(), pv.cpu().numpy())[0]
    assert np.abs(dW1 - ref.cpu().numpy()).max() <= 1e-12 * np.abs(dW1).max()
    # token bias gradients: row sums over images and channels of either operand
    for x, rows in ((p, M), (q, N)):
        xv = x[:, :rows].double()
        s, chunks = _rowsum(x, rows, D, B, torch.full((rows,), float('nan'), device='cuda'))
        assert torch.isfinite(s).all()
        ratio = ((s.double() - xv.sum((0, 2))).abs() / ((B * D + chunks) * U32 * xv.abs().sum((0, 2)))).max().item()
        print('token rowsum rows %d: worst |err| / bound = %.4f (%d chunks)' % (rows, ratio, chunks))
        assert ratio <= 1.0
        s2, _ = _rowsum(x, rows, D, B, torch.full((rows,), float('nan'), device='cuda'))
        assert torch.equal(s, s2)
        pre = torch.randn(rows, device='cuda', generator=gen)
        acc, _ = _rowsum(x, rows, D, B, pre.clone(), accumulate=1)
        assert torch.equal(acc, pre + s)


def _model(depth, seed=3):
    from robustart_amd.model.mixer_torch import MlpMixer
    torch.manual_seed(seed)
    m = MlpMixer(num_classes=1000, depth=depth)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                                   # tests/test_mixer_gpu.py::_randomize: trained-network magnitudes
        for name, p in m.named_parameters():
            if p.dim() == 1 and 'norm' in name:
                p.copy_((1.0 if name.endswith('weight') else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith('bias'):
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    return m.cuda().train()


def _compare(named_ref, grads):
    rep = []
    for (n, p), q in zip(named_ref, grads):
        ga, gb = q.double().flatten(), p.grad.double().flatten()
        rep.append((float((ga @ gb) / (ga.norm() * gb.norm() + 1e-300)), float(ga.norm() / (gb.norm() + 1e-300)), n))
    rep.sort()
    return rep


def _engine_vs_autograd(depth, B):
    from robustart_amd.model.mixer_train_engine import MixerTrainEngine
    from robustart_amd.train.arena import label_smooth_ce
    model = _model(depth)
    ref = copy.deepcopy(model)
    for p in model.parameters():
        p.grad = torch.full_like(p, float('nan'))
    ready = []
    eng = MixerTrainEngine(model, 'cuda', on_grad_ready=lambda p: ready.append(id(p)))
    x01 = torch.rand(B, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (B,), device='cuda')
    logits = eng.forward(x01, False, MEAN, STD)
    loss_rows, dl = label_smooth_ce(logits, y, 0.1, 1.0 / B)
    eng.backward(dl)
    assert len(ready) == len(set(ready)) and sorted(ready) == sorted(id(p) for p in model.parameters())
    assert len(ready) == 6 + 12 * depth
    grads = [p.grad.clone() for p in model.parameters()]
    assert all(torch.isfinite(g).all() for g in grads)
    mean = torch.tensor(MEAN, device='cuda').view(1, 3, 1, 1)
    std = torch.tensor(STD, device='cuda').view(1, 3, 1, 1)
    out = ref((x01 - mean) / std)
    loss = F.cross_entropy(out, y, label_smoothing=0.1)
    loss.backward()
    a, b = logits.double().flatten(), out.detach().double().flatten()
    cos = float((a @ b) / (a.norm() * b.norm()))
    dloss = abs(loss_rows.mean().item() - loss.item())
    rep_all = _compare(ref.named_parameters(), grads)
    null = [r for r in rep_all if r[2].endswith('.mlp_tokens.fc2.bias')]            # exact gradient zero: see the module docstring
    rep = [r for r in rep_all if not r[2].endswith('.mlp_tokens.fc2.bias')]
    assert len(null) == depth and len(rep) == 6 + 11 * depth
    cs = np.array([c for c, _, _ in rep])
    tok = [r for r in rep if '.mlp_tokens.' in r[2]]
    assert len(tok) == 3 * depth
    # torch's own bf16 autocast autograd of the same module against the fp32 run: the yardstick for a missed bar
    amp = copy.deepcopy(ref)
    amp.zero_grad()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out_amp = amp((x01 - mean) / std)
    F.cross_entropy(out_amp.float(), y, label_smoothing=0.1).backward()
    rep_amp_all = _compare(ref.named_parameters(), [p.grad for p in amp.parameters()])
    rep_amp = [r for r in rep_amp_all if not r[2].endswith('.mlp_tokens.fc2.bias')]
    null_amp = [r for r in rep_amp_all if r[2].endswith('.mlp_tokens.fc2.bias')]
    ca = np.array([c for c, _, _ in rep_amp])

    def null_distance(model_grads):
        """L2 distance to the fp32 gradient over the class mlp_tokens.fc2.bias"""
        return float(sum(((g.double() - p.grad.double()) ** 2).sum().item() for (n, p), g in zip(ref.named_parameters(), model_grads)
                         if n.endswith('.mlp_tokens.fc2.bias')) ** 0.5)
    dist_eng, dist_amp = null_distance(grads), null_distance([p.grad for p in amp.parameters()])
    scale = float(sum((p.grad.double() ** 2).sum().item() for n, p in ref.named_parameters() if n.endswith('.mlp_tokens.fc1.bias')) ** 0.5)
    null_ref = float(sum((p.grad.double() ** 2).sum().item() for n, p in ref.named_parameters() if n.endswith('.mlp_tokens.fc2.bias')) ** 0.5)
    print('Mixer depth %d B=%d, mlp_tokens.fc2.bias (exact gradient zero, |fp32 gradient| %.4e): L2 distance to the fp32 gradient: engine '
          '%.4e, torch bf16 autocast %.4e (|fp32 gradient of the fc1 biases| %.4e); cosine engine %.4f..%.4f autocast %.4f..%.4f; norm ratio engine up to '
          '%.1f, autocast up to %.1f' % (depth, B, null_ref, dist_eng, dist_amp, scale, min(c for c, _, _ in null), max(c for c, _, _ in null),
                                         min(c for c, _, _ in null_amp), max(c for c, _, _ in null_amp), max(r for _, r, _ in null),
                                         max(r for _, r, _ in null_amp)))
    aa = out_amp.detach().double().flatten()
    print('Mixer depth %d B=%d: logits cos %.7f (autocast %.7f), |dloss| %.2e of %.4f; gradient cos median %.6f min %.6f '
          '(autocast median %.6f min %.6f); norm ratio %.4f..%.4f (autocast %.4f..%.4f); lowest %s; token lowest %s'
          % (depth, B, cos, float((aa @ b) / (aa.norm() * b.norm())), dloss, loss.item(), np.median(cs), cs.min(), np.median(ca),
             ca.min(), min(r for _, r, _ in rep), max(r for _, r, _ in rep), min(r for _, r, _ in rep_amp),
             max(r for _, r, _ in rep_amp), [(round(c, 5), round(r, 4), n) for c, r, n in rep[:4]],
             [(round(c, 5), round(r, 4), n) for c, r, n in sorted(tok)[:2]]))
    assert cos > 0.99997 and dloss < 1e-3 * loss.item()
    assert np.median(cs) > 0.999 and cs.min() > 0.99, rep[:8]
    assert all(0.97 < r < 1.03 for _, r, _ in rep), [x for x in rep if not 0.97 < x[1] < 1.03][:8]
    assert dist_eng <= dist_amp, 'mlp_tokens.fc2.bias: engine %.4e farther from the fp32 gradient than bf16 autocast %.4e' % (dist_eng, dist_amp)
    # backward again from the same forward: bit-identical gradients, every parameter announced once more
    ready.clear()
    eng.backward(dl)
    assert len(ready) == len(grads) and len(set(ready)) == len(grads)
    for p, q in zip(model.parameters(), grads):
        assert torch.equal(p.grad, q)


def test_train_engine_reduced_depth_matches_torch_autograd():
    _engine_vs_autograd(2, 4)


def test_train_engine_mixer_b16_matches_torch_autograd():
    _engine_vs_autograd(12, 2)


def test_one_hip_adamw_step_matches_torch_adamw_and_repack_follows():
    from robustart_amd.model.mixer_train_engine import MixerTrainEngine
    from robustart_amd.train.arena import HipOptimizer, ParamArena, label_smooth_ce
    model = _model(2, seed=7)
    ref = copy.deepcopy(model)
    arena = ParamArena(model)
    opt = HipOptimizer(arena, kind='AdamW', lr=1e-3, weight_decay=0.05, betas=(0.9, 0.999), eps=1e-8)
    eng = MixerTrainEngine(model, 'cuda', on_grad_ready=arena.grad_ready)
    B = 4
    x01 = torch.rand(B, 3, 224, 224, device='cuda')
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
    print('Mixer AdamW step: update cosine %.5f, worst parameter difference %.2e (lr 1e-3)' % (cos, worst))
    assert cos > 0.99 and worst <= 2.0e-3 + 1e-6
    eng.repack()
    out = eng.forward(x01, False, MEAN, STD)
    assert torch.isfinite(out).all()
    fresh = MixerTrainEngine(model, 'cuda').forward(x01, False, MEAN, STD)
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
    """exprs/nips_benchmark/pgd_adv_train/mixer_B16_224/config.yaml (AdamW wd 0.05, no_wd fc / norm False, label smoothing 0.1, EMA
    0.9999, drop rates 0.0, its learning rates) on fake data, plus a 2-step PGD inner loop"""
    return {'model': {'type': 'mixer_b16_224', 'kwargs': {'drop_path': 0.0, 'drop_path_rate': 0.0}},
            'optimizer': {'type': 'AdamW', 'no_wd': {'fc': False, 'norm': False}, 'kwargs': {'weight_decay': 0.05}},
            'lr_scheduler': {'kwargs': {'base_lr': 0.000001, 'warmup_lr': 0.001, 'min_lr': 0.00001, 'warmup_steps': 1}},
            'label_smooth': 0.1, 'ema': {'enable': True, 'kwargs': {'decay': 0.9999}}, 'max_iter': 2,
            'adv_train': {'eps': '4/255', 'steps': 2},
            'data': {'read_from': 'fake', 'fake_size': 8, 'batch_size': 4, 'input_size': 224},
            'saver': dict(save_dir=save_dir, print_freq=100, **saver)}


def test_cls_solver_adversarially_trains_mixer_b16_224(tmp_path, monkeypatch):
    from robustart_amd.model.engine import EngineModel
    from robustart_amd.model.mixer_train_engine import MixerTrainEngine
    from robustart_amd.train import cls_solver as S
    built, refolds = [], []
    init, refold = MixerTrainEngine.__init__, EngineModel.rart_refold

    def spy_init(self, model, *a, **k):
        built.append(type(model).__name__)
        init(self, model, *a, **k)

    def spy_refold(self, torch_model=None):
        refold(self, torch_model)
        refolds.append(type(self.rart_engine).__name__)
    monkeypatch.setattr(MixerTrainEngine, '__init__', spy_init)
    monkeypatch.setattr(EngineModel, 'rart_refold', spy_refold)
    rank, world, device = S.init_dist()
    torch.manual_seed(5)
    loss, m_full = S.train(_solver_cfg(str(tmp_path / 'full')), _Args(), rank, world, device)
    print('mixer_b16_224 adversarial training, 2 iterations: last loss %.4f' % loss)
    assert np.isfinite(loss) and loss > 0
    assert built == ['MlpMixer']                    # MixerTrainEngine built once
    assert refolds == ['MixerEngine']               # the attack engine is refolded from the live weights at iteration 2
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
    assert any('.mlp_tokens.' in k for k in ck_a['ema'])
    for k in ck_a['ema']:
        assert torch.equal(ck_a['ema'][k], ck_b['ema'][k]), k


def test_train_step_makes_no_device_to_host_read():
    from robustart_amd.model.mixer_train_engine import MixerTrainEngine
    from robustart_amd.train.arena import label_smooth_ce
    model = _model(2)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    eng = MixerTrainEngine(model, 'cuda')
    B = 2
    x01 = torch.rand(B, 3, 224, 224, device='cuda')
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
