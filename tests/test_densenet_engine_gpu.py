"""DenseNet on DenseNetEngine: logits against the plain module in both precisions, the gradient to the input against an fp64 backward
that uses the engine's own ReLU / max-pool decisions (the method and the bounds of tests/test_resnet_family_engine_gpu.py, restated for
the pre-activation / dense-concatenation chain), the launches the chain issues, real-size cases, and a PGD run through EngineModel.
Measured errors are printed beside their bounds."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
# (2, 2, 2, 2): prefixes 64 / 96 everywhere, a 128-wide head; (6, 4, 2, 2): prefixes 64 .. 224, transition widths 128 / 128 / 96 and a 160-wide head
CONFIGS = {'2222': (2, 2, 2, 2), '6422': (6, 4, 2, 2)}


def _tiny(kind, seed=0):
    from robustart_amd.model.densenet_torch import DenseNet, randomize_bn_stats
    torch.manual_seed(seed)
    m = randomize_bn_stats(DenseNet(CONFIGS[kind], num_classes=10), seed).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


_cache = {}


def _setup(kind, precision):
    """-> (module on the host, engine), built once per (kind, precision)"""
    from robustart_amd.model.densenet_engine import DenseNetEngine
    key = (kind, precision)
    if key not in _cache:
        if kind not in _cache:
            _cache[kind] = _tiny(kind)
        _cache[key] = DenseNetEngine(_cache[kind], 'cuda', precision=precision)
    return _cache[kind], _cache[key]


def _module_logits(m, x, dtype):
    mean = torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    mm = copy.deepcopy(m).to(dtype)
    with torch.no_grad():
        return mm((x.cpu().to(dtype) - mean) / std)


def _check_logits(tag, got, m, x, precision):
    got = got.cpu().double()
    if precision == 'fp32x':
        ref64 = _module_logits(m, x, torch.float64)
        scale = ref64.abs().max().item()
        err = (got - ref64).abs().max().item() / scale
        print('%s: |engine - fp64 module| %.2e of scale %.3f  bound 1e-4' % (tag, err, scale))
        assert err <= 1e-4, tag
        assert torch.equal(got.argmax(1), ref64.argmax(1)), tag
    else:
        ref32 = _module_logits(m, x, torch.float32).double()
        scale = ref32.abs().max().item()
        err = (got - ref32).abs().max().item() / scale
        print('%s: |engine - fp32 module| %.2e of scale %.3f  bound 5e-2' % (tag, err, scale))
        assert err <= 0.05, tag


def _sign(t, dt=torch.float64):
    return torch.from_numpy(np.unpackbits(t.cpu().numpy(), axis=-1, bitorder='little')).permute(0, 3, 1, 2).to(dt)


def _reference_backward(m, eng, acts, dl, std, x3):
    """fp64 backward-to-input with the ENGINE's forward decisions (1-bit sign tensors of every pre-activation and of conv1's output,
    max-pool argmax codes).  Reference precision: the fp32 weights, nothing rounded; bf16: the bf16 tables, every gradient rounded to
    bf16 where the engine stores it (the dense temporaries, and the block's gradient buffer after every accumulation)."""
    dt = torch.float64
    q = (lambda t: t) if x3 else (lambda t: t.to(torch.bfloat16).to(dt))
    wq = (lambda w: w.cpu().to(dt)) if x3 else (lambda w: w.cpu().to(torch.bfloat16).to(dt))

    def dgrad(w, c, dz, in_hw):
        return torch.nn.grad.conv2d_input((dz.shape[0], c.cin, in_hw[0], in_hw[1]), wq(w), dz, stride=c.stride, padding=c.pad)
    B = dl.shape[0]
    if x3:
        dpool = dl.detach().cpu().to(dt) @ m.classifier.weight.detach().cpu().to(dt)
    else:
        dpool = q(q(dl.detach().cpu().to(dt)) @ eng.fc_w[:eng.n_classes].cpu().to(dt))
    _, lhw = acts['last']
    last = _sign(acts['last_sign'])
    d5 = q(last * dpool.view(B, -1, 1, 1) / (lhw[0] * lhw[1]))
    g = q(last * eng.norm5.s_host.to(dt).view(1, -1, 1, 1) * d5)
    geo = acts['geometry']
    for i in range(len(geo) - 1, -1, -1):
        hw, c0, ctot = geo[i]
        if i + 1 < len(geo):         # transition i: conv^T on the pooled rows (norm's scale in the table), d / 4 under the bits
            pre, ct = eng.trans[i]
            dtr = q(dgrad(ct.ws_folded, ct, g[:, :geo[i + 1][1]], geo[i + 1][0]))
            g = q(_sign(acts['t%d' % i]) * F.interpolate(dtr, scale_factor=2, mode='nearest') / 4)
        assert g.shape[1:] == (ctot, hw[0], hw[1])
        for j in range(len(eng.dense[i]) - 1, -1, -1):
            pre, ca, cb = eng.dense[i][j]
            sx, sa = acts['d%d_%d' % (i, j)]
            cl = c0 + j * eng.growth
            dza = q(dgrad(cb.w_folded, cb, g[:, cl:cl + eng.growth], hw) * _sign(sa))
            dop = q(dgrad(ca.ws_folded, ca, dza, hw))
            g = torch.cat([q(g[:, :cl] + _sign(sx) * dop), g[:, cl:]], 1)
    dz = g[:, :geo[0][1]]
    codes = acts['p1_argmax'].cpu().long().permute(0, 3, 1, 2)      # code k = window element (k / 3, k % 3); 15 = window maximum <= 0
    h2, w2 = codes.shape[2], codes.shape[3]
    dz1 = torch.zeros(B, codes.shape[1], 2 * h2, 2 * w2, dtype=dt)
    for k in range(9):
        ky, kx = divmod(k, 3)
        ys, xs = 2 * torch.arange(h2) - 1 + ky, 2 * torch.arange(w2) - 1 + kx
        oky, okx = ys >= 0, xs >= 0
        sel = ((codes == k).to(dt) * dz)[:, :, oky][:, :, :, okx]
        dz1[:, :, ys[oky][:, None], xs[okx][None, :]] += sel
    gi = dgrad(eng.stem.w_folded, eng.stem, q(dz1), (dz1.shape[2] * 2, dz1.shape[3] * 2))
    return gi / torch.tensor(std, dtype=dt).view(1, 3, 1, 1)


def _grad_errors(grad, ref):
    a, b = grad.double().cpu().flatten(1), ref.flatten(1)
    return ((a - b).norm(dim=1) / b.norm(dim=1)), ((a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1)))


def _check_grad(tag, grad, ref, x3):
    rel, cos = _grad_errors(grad, ref)
    if x3:
        print('%s: rel L2 %s (bound 5e-4), 1 - cos %s (bound 2e-7)' % (tag, rel.tolist(), (1 - cos).tolist()))
        assert (rel <= 5e-4).all() and (cos >= 1 - 2e-7).all(), tag
    else:
        print('%s: rel L2 %s (bound 0.03), cos %s (bound 0.9995)' % (tag, rel.tolist(), cos.tolist()))
        assert (rel < 0.03).all() and (cos > 0.9995).all(), tag


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
@pytest.mark.parametrize('HW', [64, 96])
@pytest.mark.parametrize('kind', sorted(CONFIGS))
def test_tiny_module_logits(kind, HW, precision):
    m, eng = _setup(kind, precision)
    x = torch.rand(3, 3, HW, HW, generator=torch.Generator().manual_seed(HW)).cuda()
    logits = eng.logits(x, MEAN, STD)
    _check_logits('%s %s %dx%d logits' % (kind, precision, HW, HW), logits, m, x, precision)
    assert eng.fc_in == {'2222': 128, '6422': 160}[kind] and len(eng.trans) == 3
    # the uint8 entrance: the same pixels as bytes give the logits of the fp32 entrance on x / 255
    u8 = torch.randint(0, 256, (3, HW, HW, 3), generator=torch.Generator().manual_seed(HW), dtype=torch.int32).to(torch.uint8).cuda()
    a = eng.logits_from_u8(u8, MEAN, STD)
    b = eng.logits((u8.float() / 255).permute(0, 3, 1, 2).contiguous(), MEAN, STD)
    d = (a - b).abs().max().item() / b.abs().max().item()
    print('%s %s %dx%d: logits_from_u8 vs logits %.2e of scale (bound 5e-2 / 1e-4)' % (kind, precision, HW, HW, d))
    assert d <= (1e-4 if precision == 'fp32x' else 0.05)


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
@pytest.mark.parametrize('HW', [64, 96])
@pytest.mark.parametrize('loss_kind', [0, 4])
@pytest.mark.parametrize('kind', sorted(CONFIGS))
def test_tiny_module_gradient_vs_fp64_with_the_engines_decisions(kind, loss_kind, HW, precision):
    m, eng = _setup(kind, precision)
    x3 = precision == 'fp32x'
    g = torch.Generator().manual_seed(21 + loss_kind)
    B = 3          # 64 x 64: 16 / 8 / 4 / 2 pixel sides; 96 x 96: 24 / 12 / 6 / 3, partial tiles in every launch
    x = torch.rand(B, 3, HW, HW, generator=g).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    yt = ((y + 1 + torch.randint(0, 8, (B,), generator=g).cuda()) % 10) if loss_kind == 4 else None
    logits, loss, grad, pred = eng.forward_backward(x, MEAN, STD, y, loss_kind, yt)
    tag = '%s %s %dx%d loss kind %d' % (kind, precision, HW, HW, loss_kind)
    _check_logits(tag + ' logits', logits, m, x, precision)
    assert torch.equal(pred.long(), logits.argmax(1))
    assert grad.shape == x.shape and grad.dtype == torch.float32
    ref = _reference_backward(m, eng, eng.last_acts, eng.last_dlogits, STD, x3)
    _check_grad(tag + ' gradient (engine decisions)', grad, ref, x3)


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
def test_the_chain_issues_the_densenet_launches(precision):
    """profile records of one gradient evaluation of the (6, 4, 2, 2) module: a pre-activation per dense layer and for norm5, their
    backwards, a pooled pair per transition and the two slice copies at the stem; every GEMM on the shared entries"""
    m, eng = _setup('6422', precision)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    eng.profile = []
    try:
        eng.forward_backward(x, MEAN, STD, torch.tensor([1, 2]).cuda(), 0)
        kinds = [r[3] for r in eng.profile]
    finally:
        eng.profile = None
    n = sum(CONFIGS['6422'])
    assert kinds.count('dn_preact') == n + 1 and kinds.count('dn_preact_bwd') == n + 1
    assert kinds.count('dn_preact_pool2') == 3 and kinds.count('dn_preact_pool2_bwd') == 3 and kinds.count('dn_copy') == 2
    gemms = [k for k in kinds if k in ('igemm', 'gemm_pair')]
    assert len(gemms) >= 4 * n + 6        # conv1, conv2 and their transposes per layer; a 1x1 and its transpose per transition
    with pytest.raises(NotImplementedError, match='evaluation only'):
        eng.refold(m)


@pytest.mark.parametrize('mtype,precision', [('densenet121', 'bf16'), ('densenet121', 'fp32x'), ('densenet201', 'bf16')])
def test_real_size_logits(mtype, precision):
    from robustart_amd.model import get_model
    from robustart_amd.model.densenet_engine import DenseNetEngine
    from robustart_amd.model.densenet_torch import randomize_bn_stats
    from robustart_amd.model.engine import make_engine
    torch.manual_seed(0)
    m = randomize_bn_stats(get_model({'type': mtype})).eval()
    eng = make_engine(m, 'cuda', precision)
    assert isinstance(eng, DenseNetEngine)
    x = torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)).cuda()
    _check_logits('%s %s B = 2 224 x 224 logits' % (mtype, precision), eng.logits(x, MEAN, STD), m, x, precision)


def test_pgd_linf_through_engine_model_on_densenet121():
    from robustart_amd.model import get_model
    from robustart_amd.model.densenet_engine import DenseNetEngine
    from robustart_amd.model.engine import EngineModel
    from robustart_amd.noise import AddNoise
    torch.manual_seed(0)
    model = get_model({'type': 'densenet121'}).eval()
    f = EngineModel(model, takes_normalized=False)
    assert isinstance(f.rart_engine, DenseNetEngine)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 1000, (2,), generator=g).cuda()
    eps = 4 / 255
    a = AddNoise('pgd_linf')
    a.set_config(f_model=f, eps=eps, steps=3)
    xa = a.add_noise(x, y)
    xa = xa if torch.is_tensor(xa) else torch.as_tensor(xa)
    xa = xa.to(x.device).float()
    assert xa.shape == x.shape
    assert (xa - x).abs().max().item() <= eps + 1e-6 and xa.min().item() >= 0 and xa.max().item() <= 1
    # the loss of the network itself, in fp64 on the host: the attack's gain is not mixed with the storage noise of the engine's logits
    m64 = copy.deepcopy(model).double()
    mean, std = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    with torch.no_grad():
        before, after = (F.cross_entropy(m64((t.cpu().double() - mean) / std), y.cpu(), reduction='none') for t in (x, xa))
    print('pgd_linf on densenet121: loss %s -> %s' % (before.tolist(), after.tolist()))
    assert (after >= before).all()
    ref = f.rart_reference_engine()
    assert isinstance(ref, DenseNetEngine) and ref.precision == 'bf16x3'


def test_cls_solver_evaluates_densenet121_clean_corrupted_and_under_pgd():
    """the evaluation scaffold of cls_solver takes the type unchanged: clean, one corruption, and pgd_linf at eps 4/255 on fake data"""
    from robustart_amd.train import cls_solver as S

    class A:
        engine, corruption, attack, eps, steps, severity, seed, max_iter = 'hip', None, None, '4/255', 3, 3, 0, 2
    cfg = {'model': {'type': 'densenet121', 'kwargs': {'num_classes': 1000}},
           'data': {'fake_size': 6, 'batch_size': 6, 'input_size': 224, 'read_from': 'fake'}}
    rank, world, device = S.init_dist()
    a = A()
    res = S.evaluate(cfg, a, rank, world, device)
    assert res['count'] == 6 and 0.0 <= res['top1'] <= res['top5'] <= 1.0
    a.corruption = 'gaussian_noise'
    res = S.evaluate(cfg, a, rank, world, device)
    assert res['count'] == 6 and res['noise'] == 'gaussian_noise'
    a.corruption, a.attack = None, 'pgd_linf'
    res = S.evaluate(cfg, a, rank, world, device)
    assert res['count'] == 6 and res['noise'] == 'pgd_linf'
