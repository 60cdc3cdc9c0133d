"""ResNet-18 / ResNet-34 on BasicResNetEngine: logits against the plain module in both precisions, the gradient to the input against an
fp64 backward that uses the engine's own ReLU / max-pool decisions (the method and the bounds of tests/test_resnet_family_engine_gpu.py),
in bf16 on both routes -- the fused BasicBlock kernel (csrc/basic_block.hip) and conv by conv (`basic_block_kernel = False`) -- the
real-size types, a PGD run through EngineModel, cls_solver's evaluation, and ResNet-50 never taking the new entry.  Measured errors are
printed beside their bounds."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from robustart_amd.model.basic_resnet_engine import BASIC_BLOCK_SERVED as SERVED, BASIC_BLOCK_WIDTHS as DEFAULT

pytestmark = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
LAYERS = {'1111': (1, 1, 1, 1), '2211': (2, 2, 1, 1)}
_cache = {}


def _setup(kind, precision):
    """-> (module on the host, engine), built once per (kind, precision)"""
    from robustart_amd.model.basic_resnet_engine import BasicResNetEngine
    from robustart_amd.model.resnet_basic_torch import BasicResNet
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    if kind not in _cache:
        torch.manual_seed(len(kind) + sum(LAYERS[kind]))
        m = randomize_bn_stats(BasicResNet(LAYERS[kind], num_classes=10)).eval()
        for p in m.parameters():
            p.requires_grad_(False)
        _cache[kind] = m
    if (kind, precision) not in _cache:
        _cache[(kind, precision)] = BasicResNetEngine(_cache[kind], 'cuda', precision=precision)
    return _cache[kind], _cache[(kind, precision)]


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
    """fp64 backward-to-input with the ENGINE's forward decisions (1-bit ReLU sign tensors, max-pool argmax codes).  Reference
    precision: the fp32 weights, nothing rounded; bf16: the bf16 weights, every gradient rounded to bf16 where the engine stores it (the
    fused kernel rounds the intermediate gradient where the conv-by-conv route stores it)."""
    dt = torch.float64
    q = (lambda t: t) if x3 else (lambda t: t.to(torch.bfloat16).to(dt))

    def dgrad(c, dz, in_hw):
        w = c.w_folded.cpu()
        w = w.to(dt) if x3 else w.to(torch.bfloat16).to(dt)
        return torch.nn.grad.conv2d_input((dz.shape[0], c.cin, in_hw[0], in_hw[1]), w, dz, stride=c.stride, padding=c.pad)
    B = dl.shape[0]
    if x3:
        dpool = dl.detach().cpu().to(dt) @ m.fc.weight.detach().cpu().to(dt)
    else:
        dpool = q(q(dl.detach().cpu().to(dt)) @ eng.fc_w[:eng.n_classes].cpu().to(dt))
    xl, xlhw = acts['last']
    dz = q(_sign(acts['last_sign']) * dpool.view(B, -1, 1, 1) / (xlhw[0] * xlhw[1]))
    for bi in range(len(eng.basic) - 1, -1, -1):
        c1, c2, ds = eng.basic[bi]
        _, xhw, ohw, mx, ma = acts['b%d' % bi]
        dza = q(dgrad(c2, dz, ohw) * _sign(ma))
        if ds is None:
            dz = q((dgrad(c1, dza, xhw) + dz) * _sign(mx))
        elif x3:
            dz = (dgrad(c1, dza, xhw) + dgrad(ds, dz, xhw)) * _sign(mx)
        else:
            dx = q(dgrad(c1, dza, xhw) * _sign(mx))
            dz = q((dx + dgrad(ds, dz, xhw)) * _sign(mx))
    codes = acts['p1_argmax'].cpu().long().permute(0, 3, 1, 2)      # code k = window element (k / 3, k % 3); 15 = window maximum <= 0
    h2, w2 = codes.shape[2], codes.shape[3]
    dz1 = torch.zeros(B, codes.shape[1], 2 * h2, 2 * w2, dtype=dt)
    for k in range(9):
        ky, kx = divmod(k, 3)
        ys, xs = 2 * torch.arange(h2) - 1 + ky, 2 * torch.arange(w2) - 1 + kx
        oky, okx = ys >= 0, xs >= 0
        sel = ((codes == k).to(dt) * dz)[:, :, oky][:, :, :, okx]
        dz1[:, :, ys[oky][:, None], xs[okx][None, :]] += sel
    g = dgrad(eng.stem, q(dz1), (dz1.shape[2] * 2, dz1.shape[3] * 2))
    return g / torch.tensor(std, dtype=dt).view(1, 3, 1, 1)


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
        assert (rel <= 0.03).all() and (cos >= 0.9995).all(), tag


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
@pytest.mark.parametrize('HW', [64, 96])
@pytest.mark.parametrize('kind', sorted(LAYERS))
def test_tiny_module_logits(kind, HW, precision):
    m, eng = _setup(kind, precision)
    x = torch.rand(3, 3, HW, HW, generator=torch.Generator().manual_seed(HW)).cuda()
    for switch in ((True, False) if precision == 'bf16' else (True,)):
        eng.basic_block_kernel, eng.basic_block_widths = switch, SERVED      # every width the kernel serves, whatever the default list
        try:
            got = eng.logits(x, MEAN, STD)
        finally:
            eng.basic_block_kernel, eng.basic_block_widths = True, DEFAULT
        _check_logits('%s %s %dx%d basic_block_kernel=%s logits' % (kind, precision, HW, HW, switch), got, m, x, precision)


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
@pytest.mark.parametrize('HW', [64, 96])
@pytest.mark.parametrize('loss_kind', [0, 4])
@pytest.mark.parametrize('kind', sorted(LAYERS))
def test_tiny_module_gradient_vs_fp64_with_the_engines_decisions(kind, loss_kind, HW, precision):
    """... in bf16 on both routes: each meets the bounds against its own decisions, and the two gradients differ from each other by no
    more than the bound allows"""
    m, eng = _setup(kind, precision)
    x3 = precision == 'fp32x'
    g = torch.Generator().manual_seed(21 + loss_kind)
    B = 3
    x = torch.rand(B, 3, HW, HW, generator=g).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    yt = ((y + 1 + torch.randint(0, 8, (B,), generator=g).cuda()) % 10) if loss_kind == 4 else None
    out = {}
    for switch in ((True, False) if not x3 else (True,)):
        eng.basic_block_kernel, eng.basic_block_widths, eng.profile = switch, SERVED, []
        try:
            logits, loss, grad, pred = eng.forward_backward(x, MEAN, STD, y, loss_kind, yt)
            kinds = [r[3] for r in eng.profile]
        finally:
            eng.basic_block_kernel, eng.basic_block_widths, eng.profile = True, DEFAULT, None
        n_identity = sum(ds is None for _, _, ds in eng.basic[:sum(LAYERS[kind][:2])])
        assert kinds.count('basic_block') == (2 * n_identity if (switch and not x3) else 0)
        tag = '%s %s %dx%d loss kind %d basic_block_kernel=%s' % (kind, precision, HW, HW, loss_kind, switch)
        _check_logits(tag + ' logits', logits, m, x, precision)
        assert torch.equal(pred.long(), logits.argmax(1))
        ref = _reference_backward(m, eng, eng.last_acts, eng.last_dlogits, STD, x3)
        _check_grad(tag + ' gradient (engine decisions)', grad, ref, x3)
        out[switch] = (logits.clone(), grad.clone())
    if not x3:
        dl = (out[True][0] - out[False][0]).abs().max().item() / out[False][0].abs().max().item()
        rel, cos = _grad_errors(out[True][1], out[False][1].double().cpu())
        print('%s bf16 %dx%d loss kind %d: fused vs conv by conv: logits %.2e of scale (bound 5e-2), gradient rel L2 %s (bound 0.03), cos %s '
              '(bound 0.9995)' % (kind, HW, HW, loss_kind, dl, rel.tolist(), cos.tolist()))
        assert dl <= 0.05 and (rel <= 0.03).all() and (cos >= 0.9995).all()


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
@pytest.mark.parametrize('mtype', ['resnet18_official', 'resnet34_official'])
def test_real_size_logits(mtype, precision):
    from robustart_amd.model import get_model
    from robustart_amd.model.basic_resnet_engine import BasicResNetEngine
    from robustart_amd.model.engine import make_engine
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    torch.manual_seed(0)
    m = randomize_bn_stats(get_model({'type': mtype})).eval()
    eng = make_engine(m, 'cuda', precision)
    assert isinstance(eng, BasicResNetEngine)
    x = torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)).cuda()
    for widths in ((SERVED, ()) if precision == 'bf16' else (DEFAULT,)):        # bf16: the fused route at every served width, and conv by conv
        eng.basic_block_widths = widths
        _check_logits('%s %s B = 2 224 x 224 basic_block_widths=%s logits' % (mtype, precision, widths), eng.logits(x, MEAN, STD), m, x, precision)


def test_pgd_linf_through_engine_model_on_resnet18():
    from robustart_amd.model import get_model
    from robustart_amd.model.basic_resnet_engine import BasicResNetEngine
    from robustart_amd.model.engine import EngineModel
    from robustart_amd.noise import AddNoise
    torch.manual_seed(0)
    model = get_model({'type': 'resnet18_official'}).eval()
    f = EngineModel(model, takes_normalized=False)
    assert isinstance(f.rart_engine, BasicResNetEngine)
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
    m64 = copy.deepcopy(model).double()
    mean, std = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    with torch.no_grad():
        before, after = (F.cross_entropy(m64((t.cpu().double() - mean) / std), y.cpu(), reduction='none') for t in (x, xa))
    print('pgd_linf on resnet18_official: loss %s -> %s' % (before.tolist(), after.tolist()))
    assert (after >= before).all()


@pytest.mark.parametrize('mtype', ['resnet18_official', 'resnet34_official'])
def test_cls_solver_evaluates_the_type_on_fake_data(mtype):
    from robustart_amd.train import cls_solver as S

    class A:
        engine, corruption, attack, eps, steps, severity, seed, max_iter = 'hip', None, None, '4/255', 3, 3, 0, 2
    cfg = {'model': {'type': mtype, 'kwargs': {'num_classes': 1000}},
           'data': {'fake_size': 6, 'batch_size': 6, 'input_size': 224, 'read_from': 'fake'}}
    rank, world, device = S.init_dist()
    res = S.evaluate(cfg, A(), rank, world, device)
    assert res['count'] == 6 and 0.0 <= res['top1'] <= res['top5'] <= 1.0


def test_resnet50_never_takes_the_new_entry():
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.model.resnet_torch import ResNet, randomize_bn_stats
    torch.manual_seed(0)
    eng = ResNet50Engine(randomize_bn_stats(ResNet((2, 2, 1, 1), num_classes=16)).eval(), 'cuda')
    eng.profile = []
    eng.forward_backward(torch.rand(2, 3, 64, 64).cuda(), MEAN, STD, torch.tensor([1, 2]).cuda(), 0)
    assert eng.profile and 'basic_block' not in [r[3] for r in eng.profile]
