"""The Bottleneck family beside ResNet-50 on ResNet50Engine: ResNeXt (conv2 on rart_conv3x3_grouped_*, csrc/conv_grouped.hip) and
Wide-ResNet (ungrouped: the launches ResNet-50 uses).  Logits against the plain module in both precisions, the gradient to the input
against an fp64 backward that uses the engine's own ReLU / max-pool decisions (the method and the bounds of tests/test_engine_gpu.py and
tests/test_engine_x3_gpu.py, restated here with `groups`), the new kernel against the same convolutions through the generic entries
(`grouped_conv_kernel = False`), real-size cases, and a PGD run through EngineModel.  Measured errors are printed beside their bounds."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _tiny(kind, seed=0):
    from robustart_amd.model.resnet_torch import ResNet, randomize_bn_stats
    torch.manual_seed(seed)
    if kind == 'grouped':       # conv2 widths 32 / 64 / 128 / 256: group widths 4, 8, 16, 32; an identity block, three stride-2 first blocks
        m = ResNet((2, 1, 1, 1), num_classes=10, groups=8, width_per_group=4)
    else:
        m = ResNet((1, 1, 1, 1), num_classes=10, width_per_group=128)
    m = randomize_bn_stats(m, seed).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


_cache = {}


def _setup(kind, precision):
    """-> (module on the host, engine), built once per (kind, precision)"""
    from robustart_amd.model.engine import ResNet50Engine
    key = (kind, precision)
    if key not in _cache:
        if kind not in _cache:
            _cache[kind] = _tiny(kind)
        _cache[key] = ResNet50Engine(_cache[kind], 'cuda', precision=precision)
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
    if t.dtype == torch.uint8:
        return torch.from_numpy(np.unpackbits(t.cpu().numpy(), axis=-1, bitorder='little')).permute(0, 3, 1, 2).to(dt)
    return (t.detach().cpu().to(dt).permute(0, 3, 1, 2) > 0).to(dt)


def _reference_backward(m, eng, acts, dl, std, x3):
    """fp64 backward-to-input with the ENGINE's forward decisions (1-bit ReLU sign tensors, max-pool argmax codes).  Reference
    precision: the fp32 weights, nothing rounded (tests/test_engine_x3_gpu.py); bf16: the bf16 weights, every gradient rounded to bf16
    where the engine stores it (tests/test_engine_gpu.py).  Grouped convolutions pass `groups`."""
    dt = torch.float64
    q = (lambda t: t) if x3 else (lambda t: t.to(torch.bfloat16).to(dt))

    def dgrad(c, dz, in_hw):
        w = c.w_folded.cpu()
        w = w.to(dt) if x3 else w.to(torch.bfloat16).to(dt)
        return torch.nn.grad.conv2d_input((dz.shape[0], c.cin, in_hw[0], in_hw[1]), w, dz, stride=c.stride, padding=c.pad, groups=c.groups)
    B = dl.shape[0]
    if x3:
        dpool = dl.detach().cpu().to(dt) @ m.fc.weight.detach().cpu().to(dt)
    else:
        dpool = q(q(dl.detach().cpu().to(dt)) @ eng.fc_w[:eng.n_classes].cpu().to(dt))
    xl, xlhw = acts['last']
    last = _sign(acts['last_sign']) if x3 else _sign(xl)
    dz = q(last * dpool.view(B, -1, 1, 1) / (xlhw[0] * xlhw[1]))
    for bi in range(len(eng.blocks) - 1, -1, -1):
        ca, cb, cc, ds = eng.blocks[bi]
        x, xhw, ya, yb, yc, ohw = acts['b%d' % bi]
        mx, ma, mb = acts['b%d_masks' % bi]
        dzb = q(dgrad(cc, dz, ohw) * _sign(mb))
        dza = q(dgrad(cb, dzb, xhw) * _sign(ma))
        if ds is None:
            dz = q((dgrad(ca, dza, xhw) + dz) * _sign(mx))
        elif x3:
            dz = (dgrad(ca, dza, xhw) + dgrad(ds, dz, xhw)) * _sign(mx)
        else:
            dx = q(dgrad(ca, dza, xhw) * _sign(mx))
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
        assert (rel < 0.03).all() and (cos > 0.9995).all(), tag


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
@pytest.mark.parametrize('HW', [64, 96])
@pytest.mark.parametrize('kind', ['grouped', 'wide'])
def test_tiny_module_logits(kind, HW, precision):
    m, eng = _setup(kind, precision)
    x = torch.rand(3, 3, HW, HW, generator=torch.Generator().manual_seed(HW)).cuda()
    _check_logits('%s %s %dx%d logits' % (kind, precision, HW, HW), eng.logits(x, MEAN, STD), m, x, precision)
    if kind == 'grouped':
        assert [(cb.groups, cb.gw) for _, cb, _, _ in eng.blocks] == [(8, 4), (8, 4), (8, 8), (8, 16), (8, 32)]
        assert all(getattr(cb, 'w_fwd_frag', None) is None and getattr(cc, 'tail_fwd', None) is None for _, cb, cc, _ in eng.blocks)
    else:
        assert all(cb.groups == 1 for _, cb, _, _ in eng.blocks)


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
@pytest.mark.parametrize('HW', [64, 96])
@pytest.mark.parametrize('loss_kind', [0, 4])
@pytest.mark.parametrize('kind', ['grouped', 'wide'])
def test_tiny_module_gradient_vs_fp64_with_the_engines_decisions(kind, loss_kind, HW, precision):
    """... and, for the grouped module, the switch: the new kernel and the generic entries both meet the bounds; their difference is
    printed (the accumulation order differs, so no bit identity is asked)"""
    m, eng = _setup(kind, precision)
    x3 = precision == 'fp32x'
    g = torch.Generator().manual_seed(21 + loss_kind)
    B = 3          # 64 x 64: layer1 is one 16 x 16 tile; 96 x 96: 24 / 12 / 6 / 3, partial tiles and tile boundaries in every launch
    x = torch.rand(B, 3, HW, HW, generator=g).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    yt = ((y + 1 + torch.randint(0, 8, (B,), generator=g).cuda()) % 10) if loss_kind == 4 else None
    out = {}
    for switch in ((True, False) if kind == 'grouped' else (True,)):
        eng.grouped_conv_kernel = switch
        try:
            logits, loss, grad, pred = eng.forward_backward(x, MEAN, STD, y, loss_kind, yt)
        finally:
            eng.grouped_conv_kernel = True
        tag = '%s %s %dx%d loss kind %d grouped_conv_kernel=%s' % (kind, precision, HW, HW, loss_kind, switch)
        _check_logits(tag + ' logits', logits, m, x, precision)
        assert torch.equal(pred.long(), logits.argmax(1))
        ref = _reference_backward(m, eng, eng.last_acts, eng.last_dlogits, STD, x3)
        _check_grad(tag + ' gradient (engine decisions)', grad, ref, x3)
        out[switch] = (logits.clone(), grad.clone())
    if kind == 'grouped':
        dl = (out[True][0] - out[False][0]).abs().max().item() / out[False][0].abs().max().item()
        rel, cos = _grad_errors(out[True][1], out[False][1].double().cpu())
        print('%s %s %dx%d loss kind %d: new kernel vs generic entries: logits %.2e of scale, gradient rel L2 %s'
              % (kind, precision, HW, HW, loss_kind, dl, rel.tolist()))


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
@pytest.mark.parametrize('n_classes', [10, 16, 100, 1000])
def test_classifier_head_at_class_counts_that_are_and_are_not_multiples_of_8(n_classes, precision):
    """the head's forward writes ceil8(n) columns and its backward contracts over ceil64(n): a plain (ungrouped) tiny module at 10 and
    100 classes (neither a multiple of 8), 16 and 1000 (1000: the padding ResNet-50 always had), logits and gradient by the bounds above"""
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.model.resnet_torch import ResNet, randomize_bn_stats
    torch.manual_seed(n_classes)
    m = randomize_bn_stats(ResNet((1, 1, 1, 1), num_classes=n_classes), 1).eval()
    eng = ResNet50Engine(m, 'cuda', precision=precision)
    assert eng.n_cols8 == (n_classes + 7) // 8 * 8 and eng.fc_kpad == (n_classes + 63) // 64 * 64 and eng.fc_b.shape == (n_classes,)
    g = torch.Generator().manual_seed(n_classes)
    x = torch.rand(3, 3, 64, 64, generator=g).cuda()
    y = torch.randint(0, n_classes, (3,), generator=g).cuda()
    logits, loss, grad, pred = eng.forward_backward(x, MEAN, STD, y, 0)
    tag = 'head %d classes %s' % (n_classes, precision)
    assert logits.shape == (3, n_classes) and logits.is_contiguous()
    _check_logits(tag + ' logits', logits, m, x, precision)
    assert torch.equal(pred.long(), logits.argmax(1))
    _check_grad(tag + ' gradient (engine decisions)', grad, _reference_backward(m, eng, eng.last_acts, eng.last_dlogits, STD, precision == 'fp32x'),
                precision == 'fp32x')


def test_the_switch_changes_the_launches_and_resnet50_never_takes_the_new_entry():
    """profile records: the grouped module issues 'grouped3x3' launches with the switch on and none with it off; a plain ResNet issues none"""
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.model.resnet_torch import ResNet, randomize_bn_stats
    m, eng = _setup('grouped', 'bf16')
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    y = torch.tensor([1, 2]).cuda()
    kinds = {}
    for switch in (True, False):
        eng.grouped_conv_kernel, eng.profile = switch, []
        try:
            eng.forward_backward(x, MEAN, STD, y, 0)
            kinds[switch] = [r[3] for r in eng.profile]
        finally:
            eng.grouped_conv_kernel, eng.profile = True, None
    # forward 5 launches; backward 2 identity / stride-1 blocks x 1 + 3 stride-2 blocks x 4 classes
    assert kinds[True].count('grouped3x3') == 5 + 2 + 12 and 'grouped3x3' not in kinds[False]
    torch.manual_seed(0)
    plain = ResNet50Engine(randomize_bn_stats(ResNet((1, 1, 1, 1), num_classes=16)).eval(), 'cuda')
    plain.profile = []
    plain.forward_backward(x, MEAN, STD, y, 0)
    assert 'grouped3x3' not in [r[3] for r in plain.profile]


@pytest.mark.parametrize('mtype,precision', [('resnext50_32x4d', 'bf16'), ('resnext50_32x4d', 'fp32x'), ('wide_resnet50_2', 'bf16')])
def test_real_size_logits(mtype, precision):
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import make_engine
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    torch.manual_seed(0)
    m = randomize_bn_stats(get_model({'type': mtype})).eval()
    eng = make_engine(m, 'cuda', precision)
    x = torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)).cuda()
    _check_logits('%s %s B = 2 224 x 224 logits' % (mtype, precision), eng.logits(x, MEAN, STD), m, x, precision)


def test_pgd_linf_through_engine_model_on_resnext50():
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import EngineModel
    from robustart_amd.noise import AddNoise
    torch.manual_seed(0)
    model = get_model({'type': 'resnext50_32x4d'}).eval()
    f = EngineModel(model, takes_normalized=False)
    assert f.rart_engine.blocks[0][1].groups == 32
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
    print('pgd_linf on resnext50_32x4d: loss %s -> %s' % (before.tolist(), after.tolist()))
    assert (after >= before).all()
    ref = f.rart_reference_engine()
    assert ref.precision == 'bf16x3' and ref.blocks[0][1].groups == 32
