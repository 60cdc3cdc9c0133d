"""ViT engines beyond 224 tokens: a tiny `vit_base` (width 128, two heads of 64, two blocks, 40 classes) at 256 px (257 tokens) and
384 px (577 tokens) through ViTEngine / EngineModel / ViTTrainEngine on the streaming attention entries, and at 224 px (197 tokens) as
the control: the streaming entries forced (`stream_attention = True`) against the resident route.

Bounds (those of the 224-pixel engine tests):
  reference precision: logits within 1e-4 of scale of the fp64 module on the host and of the fp32 module; input gradient (CE, DLR)
      rel L2 <= 5e-4 and cos >= 1 - 2e-7 against fp64 autograd;
  bf16: logits < 0.03 * scale, input gradient cos > 0.995 and rel < 0.1;
  control: pair logits <= 2e-5 of scale, pair gradient <= 5e-5 of scale, bf16 cos > 0.9995;
  train engine: test_vit_train_engine_parameter_gradients_match_torch_autograd's.
The fp32 and fp64 modules run on the host: torch's GPU convolution builds its kernels per image size, which costs each size tens of seconds."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CLASSES, BATCH = 40, 2
TOKENS = {224: 197, 256: 257, 384: 577}


def _module(img, train=False):
    from robustart_amd.model import get_model
    torch.manual_seed(img)
    m = get_model({'type': 'vit_base', 'kwargs': {'img_size': img, 'embed_dim': 128, 'num_heads': 2, 'depth': 2, 'num_classes': CLASSES}})
    g = torch.Generator().manual_seed(1)
    for n, p in m.named_parameters():                      # non-trivial biases / norms so that every epilogue term is exercised
        if n.endswith('bias'):
            p.data.copy_(torch.randn(p.shape, generator=g) * 0.05)
        if 'norm' in n and n.endswith('weight'):
            p.data.copy_(1 + torch.randn(p.shape, generator=g) * 0.1)
    if train:
        return m.cuda().train()
    for p in m.parameters():
        p.requires_grad_(False)
    return m.eval().cuda()


_CACHE = {}


def _setup(img):
    """(fp32 module on the host, {precision: engine}, x, y, fp64 module on the host) of one image size, built once"""
    if img not in _CACHE:
        from robustart_amd.model.vit_engine import ViTEngine
        m = _module(img)
        g = torch.Generator().manual_seed(img + 7)
        x = torch.rand(BATCH, 3, img, img, generator=g).cuda()
        y = torch.randint(0, CLASSES, (BATCH,), generator=g).cuda()
        engines = {p: ViTEngine(m, 'cuda', precision=p) for p in ('bf16', 'fp32x')}
        assert all(e.tokens == TOKENS[img] for e in engines.values())
        _CACHE[img] = (copy.deepcopy(m).cpu(), engines, x, y, copy.deepcopy(m).cpu().double())
    return _CACHE[img]


def _ref_gradient(m64, x, dl):
    """fp64 logits and d(sum logits * dl)/dx through the module on the host"""
    mean = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    xr = x.cpu().double().requires_grad_(True)
    lg = m64((xr - mean) / std)
    want, = torch.autograd.grad((lg * dl.double().cpu()).sum(), xr)
    return lg.detach().cuda(), want.cuda()


def _fp32(m, x):
    """logits of the fp32 module on the host (x may require grad), as a tensor on the host"""
    mean = torch.tensor(MEAN).view(1, 3, 1, 1)
    std = torch.tensor(STD).view(1, 3, 1, 1)
    return m((x.cpu() - mean) / std)


def _rows(a, b):
    a, b = a.double().flatten(1), b.double().flatten(1)
    return ((a - b).norm(dim=1) / b.norm(dim=1)).cpu(), ((a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).cpu()


@pytest.mark.parametrize('img', [256, 384, 224])
def test_reference_precision_engine_beyond_224_tokens(img):
    m, engines, x, y, m64 = _setup(img)
    eng = engines['fp32x']
    assert eng._streams(eng.tokens) == (img > 224)
    for kind in (0, 1):                                     # CE, DLR
        logits, loss, grad, pred = eng.forward_backward(x, MEAN, STD, y, kind)
        lg, want = _ref_gradient(m64, x, eng.last_dlogits)
        scale = lg.abs().max().item()
        e64 = (logits.double() - lg).abs().max().item() / scale
        e32 = (logits.double().cpu() - _fp32(m, x).double()).abs().max().item() / scale
        rel, cos = _rows(grad, want)
        xt = x.cpu().requires_grad_(True)
        gt, = torch.autograd.grad((_fp32(m, xt) * eng.last_dlogits.cpu()).sum(), xt)
        rel_t, _ = _rows(gt.cuda(), want)
        print('ViT x3 %d tokens kind=%d: logits vs fp64 %.2e, vs fp32 module %.2e of scale; gradient rel L2 %s (torch fp32 autograd: %s), '
              '1 - cos %s' % (eng.tokens, kind, e64, e32, rel.tolist(), rel_t.tolist(), (1 - cos).tolist()))
        assert e64 <= 1e-4 and e32 <= 1e-4
        assert (rel <= 5e-4).all() and (cos >= 1 - 2e-7).all()
        assert torch.equal(pred.long(), lg.argmax(1))


@pytest.mark.parametrize('img', [256, 384, 224])
def test_bf16_engine_beyond_224_tokens(img):
    m, engines, x, y, m64 = _setup(img)
    eng = engines['bf16']
    logits, loss, grad, pred = eng.forward_backward(x, MEAN, STD, y, 0)
    assert ('att_stats' in eng._buf) == (img > 224)
    lg, want = _ref_gradient(m64, x, eng.last_dlogits)
    scale = lg.abs().max().item()
    err = (logits.double() - lg).abs().max().item()
    a, b = grad.double().flatten(), want.flatten()
    cos, rel = (a @ b / (a.norm() * b.norm())).item(), ((a - b).norm() / b.norm()).item()
    print('ViT bf16 %d tokens: logits max err %.3g at scale %.3f; gradient 1 - cos %.2e, rel %.2e' % (eng.tokens, err, scale, 1 - cos, rel))
    assert err < 0.03 * scale
    assert cos > 0.995 and rel < 0.1


def test_stream_entries_match_the_resident_route_at_197_tokens():
    m, engines, x, y, _ = _setup(224)
    for precision, eng in engines.items():
        assert eng.stream_attention is None
        l0, _, g0, _ = [t.clone() if torch.is_tensor(t) else t for t in eng.forward_backward(x, MEAN, STD, y, 0)]
        eng.stream_attention = True
        try:
            l1, _, g1, _ = eng.forward_backward(x, MEAN, STD, y, 0)
        finally:
            eng.stream_attention = None
        el = (l1 - l0).abs().max().item() / l0.abs().max().item()
        eg = (g1 - g0).abs().max().item() / g0.abs().max().item()
        a, b = g1.double().flatten(), g0.double().flatten()
        cos = (a @ b / (a.norm() * b.norm())).item()
        print('ViT %s 197 tokens, stream vs resident: logits %.2e, gradient %.2e of scale, 1 - cos %.2e' % (precision, el, eg, 1 - cos))
        if precision == 'fp32x':
            assert el <= 2e-5 and eg <= 5e-5
        else:
            la, lb = l1.double().flatten(), l0.double().flatten()
            assert cos > 0.9995 and (la @ lb / (la.norm() * lb.norm())).item() > 0.9995


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
def test_pgd_through_engine_model_at_257_tokens(precision):
    """AddNoise('pgd_linf') with the engine as f_model: inside the eps ball and [0, 1], the loss goes up; the attack entry runs without
    a device-to-host read"""
    from robustart_amd.model.engine import EngineModel
    from robustart_amd.noise import AddNoise, adv, rng
    m, engines, x, y, _ = _setup(256)
    f = EngineModel(None, takes_normalized=False, engine=engines[precision])
    eps = 4 / 255
    rng.manual_seed(11, 0)
    an = AddNoise('pgd_linf')
    an.set_config(f_model=f, eps=eps, steps=3)
    xa = an.add_noise(x, y)
    assert (xa - x).abs().max().item() <= eps + 1e-6 and xa.min().item() >= 0 and xa.max().item() <= 1
    ce = torch.nn.functional.cross_entropy
    clean, attacked = ce(_fp32(m, x), y.cpu()).item(), ce(_fp32(m, xa), y.cpu()).item()
    print('PGD at 257 tokens (%s): CE %.4f -> %.4f' % (precision, clean, attacked))
    assert attacked > clean
    want = adv.pgd_linf(x, y, f, eps, 3 / 40, 2, seed=9, sample_offset=0)           # warm-up: allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = adv.pgd_linf(x, y, f, eps, 3 / 40, 2, seed=9, sample_offset=0)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(got, want)


def test_vit_train_engine_parameter_gradients_at_257_tokens():
    """ViTTrainEngine (backward through the engine's attention choice) vs torch autograd through the fp32 module"""
    import numpy as np
    from robustart_amd.model.vit_train_engine import ViTTrainEngine
    from robustart_amd.train.arena import label_smooth_ce
    model = _module(256, train=True)
    ref = copy.deepcopy(model).cpu()
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    ready = []
    eng = ViTTrainEngine(model, 'cuda', on_grad_ready=lambda p: ready.append(id(p)))
    B = 4
    torch.manual_seed(3)
    x01 = torch.rand(B, 3, 256, 256, device='cuda')
    y = torch.randint(0, CLASSES, (B,), device='cuda')
    logits = eng.forward(x01, False, MEAN, STD)
    _, dl = label_smooth_ce(logits, y, 0.1, 1.0 / B)
    eng.backward(dl)
    assert 'att_stats' in eng._buf
    assert sorted(ready) == sorted(id(p) for p in model.parameters())
    out = _fp32(ref, x01)
    out.backward(dl.cpu())                                        # the same upstream gradient on both sides
    assert (logits.cpu() - out.detach()).abs().max() < 0.02 * out.detach().abs().max()
    rep = []
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        a, b2 = p.grad.double().flatten().cpu(), q.grad.double().flatten()
        rep.append((float((a @ b2) / (a.norm() * b2.norm() + 1e-30)), float(a.norm() / (b2.norm() + 1e-30)), n))
    rep.sort()
    print('lowest parameter-gradient cosines at 257 tokens:', [(round(c, 4), round(r, 3), n) for c, r, n in rep[:6]])
    cs = np.array([c for c, _, _ in rep])
    assert np.median(cs) > 0.999 and cs.min() > 0.98, rep[:8]
    assert all(0.9 < r < 1.1 for _, r, _ in rep), [x for x in rep if not 0.9 < x[1] < 1.1][:8]
