"""ConvNeXt-V2-B (model `convnextv2_base`) on the HIP engine: the GRN kernels of csrc/convnext_v2.hip against fp64 of the same operands
at the four stage shapes, then the whole engine (ConvNeXtEngine with GRN blocks) in both precisions against the fp32 module and an
fp64 copy, batch invariance at B = 256 and run-to-run identity, PGD through AddNoise / EngineModel, the solver's attacked evaluation
and the attack entry under torch.cuda.set_sync_debug_mode('error').

GRN weight and bias are drawn from N(0, 0.5) everywhere: timm initialises both to zero, which makes GRN the identity.

Tolerances (as tests/test_convnext_gpu.py):
  * kernels vs fp64 of the same (bf16 / pair) operands: bf16 outputs within one bf16 rounding (2^-8 relative) + 1e-4 of the scale;
    pair outputs within 2^-15 relative + 2e-5 of the scale; the fp32 statistics G and a within 1e-5 relative + 1e-5 of the scale;
  * fp32x engine: logits within 1e-4 of max|logit| of the fp32 module AND of an fp64 copy; input gradient vs fp64 autograd:
    relative L2 <= 2e-4 per image;
  * bf16 engine vs the fp32 module: logits within 2e-2 of max|logit|, input gradient cosine >= 0.999.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HIDDEN = [(56 * 56, 512), (28 * 28, 1024), (14 * 14, 2048), (7 * 7, 4096)]     # (pixels, 4C) per stage at 224 x 224
EPS = 1e-6


def _lib():
    from robustart_amd import _lib as L
    return L, L.load()


def _split(t):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


def _val(t, pair):
    return (t[0].double() + t[1].double()) if pair else t.double()


def _make(t, pair):
    return _split(t.float()) if pair else t.to(torch.bfloat16).contiguous()


def _hl(t, pair):
    return (t[0].data_ptr(), t[1].data_ptr()) if pair else (t.data_ptr(),)


def _close(got, ref, pair, what, fp32=False):
    scale = ref.abs().max().item()
    if fp32:
        rtol, atol = 1e-5, 1e-5 * scale
    else:
        rtol, atol = (2.0 ** -15, 2e-5 * scale) if pair else (2.0 ** -8, 1e-4 * scale)
    err = (got - ref).abs()
    bad = (err > rtol * ref.abs() + atol).sum().item()
    print('%s: max |err| %.3e (scale %.3e), %d outside' % (what, err.max().item(), scale, bad))
    assert bad == 0, what


def _gelu_grad(u):
    return 0.5 * (1 + torch.erf(u / 2 ** 0.5)) + u * torch.exp(-u * u / 2) / (2 * torch.pi) ** 0.5


def _operands(B, P, C, pair, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    u = torch.randn(B, P, C, device='cuda', generator=g)
    y = F.gelu(u)
    y[1, :, 5] = 0.0                                                   # one all-zero channel: G == 0
    w = (0.5 * torch.randn(C, device='cuda', generator=g)).contiguous()
    b = (0.5 * torch.randn(C, device='cuda', generator=g)).contiguous()
    gz = torch.randn(B, P, C, device='cuda', generator=g)
    return _make(u, pair), _make(y, pair), _make(gz, pair), w, b


def _ref(uv, yv, gv, w, b):
    """fp64 GRN forward / backward (the closed form tests/test_convnext_v2_cpu.py checks against autograd)"""
    C = yv.shape[-1]
    G = torch.sqrt((yv * yv).sum(1))                                   # [B][C]
    m = G.mean(1, keepdim=True)
    z = yv * (1 + w * (G / (m + EPS)))[:, None, :] + b
    a = w * (gv * yv).sum(1)
    s = (a * G).sum(1, keepdim=True)
    beta = a / (m + EPS) - s / (C * (m + EPS) ** 2)
    ratio = torch.where(G > 0, beta / torch.where(G > 0, G, torch.ones_like(G)), torch.zeros_like(G))
    dh = (gv * (1 + w * (G / (m + EPS)))[:, None, :] + yv * ratio[:, None, :]) * _gelu_grad(uv)
    return G, z, a, dh


@pytest.mark.parametrize('pair', [False, True])
@pytest.mark.parametrize('shape', HIDDEN)
def test_grn_kernels_vs_fp64(shape, pair):
    L, lib = _lib()
    P, C = shape
    B = 2
    u, y, gz, w, b = _operands(B, P, C, pair, P + C)
    uv, yv, gv = _val(u, pair), _val(y, pair), _val(gz, pair)
    wd, bd = w.double(), b.double()
    G_ref, z_ref, a_ref, dh_ref = _ref(uv, yv, gv, wd, bd)
    assert (G_ref[1, 5] == 0).item()
    sp = L.stream_ptr()
    tag = '%s %s' % (shape, 'pair' if pair else 'bf16')
    G = torch.empty(B, C, device='cuda')
    z = torch.empty_like(y)
    a = torch.empty(B, C, device='cuda')
    dh = torch.empty_like(gz)
    sfx = 'pair' if pair else 'bf16'
    L.check(getattr(lib, 'rart_cnx_grn_stats_' + sfx)(*_hl(y, pair), G.data_ptr(), B, P, C, sp))
    L.check(getattr(lib, 'rart_cnx_grn_apply_' + sfx)(*_hl(y, pair), G.data_ptr(), w.data_ptr(), b.data_ptr(), *_hl(z, pair), B, P, C,
                                                      EPS, sp))
    L.check(getattr(lib, 'rart_cnx_grn_bwd_reduce_' + sfx)(*_hl(gz, pair), *_hl(y, pair), w.data_ptr(), a.data_ptr(), B, P, C, sp))
    L.check(getattr(lib, 'rart_cnx_grn_bwd_apply_' + sfx)(*_hl(gz, pair), *_hl(y, pair), *_hl(u, pair), G.data_ptr(), a.data_ptr(),
                                                          w.data_ptr(), *_hl(dh, pair), B, P, C, EPS, sp))
    _close(G.double(), G_ref, pair, 'GRN stats ' + tag, fp32=True)
    assert G[1, 5].item() == 0.0
    _close(_val(z, pair), z_ref, pair, 'GRN apply ' + tag)
    _close(a.double(), a_ref, pair, 'GRN bwd reduce ' + tag, fp32=True)
    _close(_val(dh, pair), dh_ref, pair, 'GRN bwd apply ' + tag)
    # in place (the engine's calls): dh over g, z over y -- the same bits
    L.check(getattr(lib, 'rart_cnx_grn_bwd_apply_' + sfx)(*_hl(gz, pair), *_hl(y, pair), *_hl(u, pair), G.data_ptr(), a.data_ptr(),
                                                          w.data_ptr(), *_hl(gz, pair), B, P, C, EPS, sp))
    L.check(getattr(lib, 'rart_cnx_grn_apply_' + sfx)(*_hl(y, pair), G.data_ptr(), w.data_ptr(), b.data_ptr(), *_hl(y, pair), B, P, C,
                                                      EPS, sp))
    assert torch.equal(gz, dh) and torch.equal(y, z)


def test_grn_statistics_do_not_depend_on_the_batch():
    """image i's G and a are the same bits in a batch of 256 and in a batch of 8 (no launch geometry depends on n)"""
    L, lib = _lib()
    P, C = HIDDEN[0]
    g = torch.Generator(device='cuda').manual_seed(1)
    y = F.gelu(torch.randn(256, P, C, device='cuda', generator=g)).to(torch.bfloat16)
    gz = torch.randn(256, P, C, device='cuda', generator=g).to(torch.bfloat16)
    w = torch.randn(C, device='cuda', generator=g)
    sp = L.stream_ptr()
    Gb, ab = torch.empty(256, C, device='cuda'), torch.empty(256, C, device='cuda')
    L.check(lib.rart_cnx_grn_stats_bf16(y.data_ptr(), Gb.data_ptr(), 256, P, C, sp))
    L.check(lib.rart_cnx_grn_bwd_reduce_bf16(gz.data_ptr(), y.data_ptr(), w.data_ptr(), ab.data_ptr(), 256, P, C, sp))
    for i in (0, 120, 248):
        Gs, as_ = torch.empty(8, C, device='cuda'), torch.empty(8, C, device='cuda')
        ys, gs = y[i:i + 8].contiguous(), gz[i:i + 8].contiguous()
        L.check(lib.rart_cnx_grn_stats_bf16(ys.data_ptr(), Gs.data_ptr(), 8, P, C, sp))
        L.check(lib.rart_cnx_grn_bwd_reduce_bf16(gs.data_ptr(), ys.data_ptr(), w.data_ptr(), as_.data_ptr(), 8, P, C, sp))
        assert torch.equal(Gs, Gb[i:i + 8]) and torch.equal(as_, ab[i:i + 8]), i


# ---------------------------------------------------------------------------------------------------------------- whole network
def _randomize(m, seed):
    """trained-network magnitudes: LayerNorm affines near 1 / 0, GRN weight and bias N(0, 0.5) (timm's zeros would hide GRN)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if '.grn.' in name:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1 and ('norm' in name or name.startswith('stem.1') or 'downsample.0' in name):
                p.copy_((1.0 if name.endswith('weight') else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith('conv_dw.weight'):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith('bias'):
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    return m.eval()


@pytest.fixture(scope='module')
def model():
    from robustart_amd.model import get_model
    torch.manual_seed(0)
    return _randomize(get_model({'type': 'convnextv2_base', 'kwargs': {'num_classes': 1000}}), 1).cuda()


@pytest.fixture(scope='module')
def engines(model):
    from robustart_amd.model.engine import make_engine
    e = {'bf16': make_engine(model, 'cuda', 'bf16'), 'fp32x': make_engine(model, 'cuda', 'fp32x')}
    assert all(x.grn for x in e.values())
    return e


def _fp64_logits_and_grad(model, x, dl):
    m64 = copy.deepcopy(model).cpu().double()
    mean = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    xr = x.cpu().double().requires_grad_(True)
    lg = m64((xr - mean) / std)
    g, = torch.autograd.grad((lg * dl.cpu().double()).sum(), xr)
    return lg.detach().cuda(), g.cuda()


def _fp32_module(model, x):
    mean = torch.tensor(MEAN, device='cuda').view(1, 3, 1, 1)
    std = torch.tensor(STD, device='cuda').view(1, 3, 1, 1)
    return model((x - mean) / std)


def test_fp32x_engine_vs_fp32_module_and_fp64(model, engines):
    eng = engines['fp32x']
    torch.manual_seed(3)
    B = 2
    x = torch.rand(B, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (B,), device='cuda')
    logits, loss, grad, pred = eng.forward_backward(x, MEAN, STD, y, 0)
    fwd = eng.logits(x, MEAN, STD)
    assert torch.equal(fwd, logits)
    dl = eng.last_dlogits.clone()
    with torch.no_grad():
        pure = _fp32_module(model, x).double()
    ref, want = _fp64_logits_and_grad(model, x, dl)
    scale = ref.abs().max().item()
    e32 = (logits.double() - pure).abs().max().item()
    e64 = (logits.double() - ref).abs().max().item()
    a, b = grad.double().flatten(1), want.flatten(1)
    rel = ((a - b).norm(dim=1) / b.norm(dim=1)).cpu()
    print('ConvNeXt-V2 fp32x: max|logit| %.4f; |engine - fp32 module| %.3e (%.2e of scale), |engine - fp64| %.3e (%.2e); '
          'input gradient rel L2 vs fp64 %s' % (scale, e32, e32 / scale, e64, e64 / scale, rel.tolist()))
    assert e32 <= 1e-4 * scale and e64 <= 1e-4 * scale
    assert (rel <= 2e-4).all()
    assert torch.equal(pred.long(), ref.argmax(1))


def test_bf16_engine_vs_fp32_module(model, engines):
    eng = engines['bf16']
    torch.manual_seed(4)
    B = 4
    x = torch.rand(B, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (B,), device='cuda')
    logits, loss, grad, pred = eng.forward_backward(x, MEAN, STD, y, 0)
    dl = eng.last_dlogits.clone()
    xt = x.clone().requires_grad_(True)
    lt = _fp32_module(model, xt)
    gt, = torch.autograd.grad((lt * dl).sum(), xt)
    scale = lt.abs().max().item()
    err = (logits - lt.detach()).abs().max().item()
    a, b = grad.double().flatten(1), gt.double().flatten(1)
    cos = ((a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).cpu()
    rel = ((a - b).norm(dim=1) / b.norm(dim=1)).cpu()
    print('ConvNeXt-V2 bf16: max|logit| %.4f, |engine - fp32 module| %.3e (%.2e of scale); gradient cos %s, rel L2 %s'
          % (scale, err, err / scale, cos.tolist(), rel.tolist()))
    assert err <= 2e-2 * scale
    assert (cos >= 0.999).all()
    f = eng.logits(x, MEAN, STD)
    assert (f - logits).abs().max().item() <= 2e-2 * scale       # forward-only fc1: GELU of the fp32 pre-activation


def test_engines_b256_match_b8_bit_for_bit_and_repeat(model, engines):
    g = torch.Generator().manual_seed(5)
    x = torch.rand(256, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 1000, (256,), generator=g).cuda()
    for name, eng in engines.items():
        big = eng.logits(x, MEAN, STD).clone()
        assert torch.equal(eng.logits(x, MEAN, STD), big), name
        lb, _, gb, _ = eng.forward_backward(x, MEAN, STD, y, 0)
        lb, gb = lb.clone(), gb.clone()
        l2, _, g2, _ = eng.forward_backward(x, MEAN, STD, y, 0)
        assert torch.equal(l2, lb) and torch.equal(g2, gb), name
        del l2, g2
        for i in (0, 120, 248):
            xs, ys = x[i:i + 8].contiguous(), y[i:i + 8].contiguous()
            assert torch.equal(eng.logits(xs, MEAN, STD), big[i:i + 8]), (name, i)
            ls, _, gs, _ = eng.forward_backward(xs, MEAN, STD, ys, 0)
            assert torch.equal(ls, lb[i:i + 8]) and torch.equal(gs, gb[i:i + 8]), (name, i)
        eng._buf.clear()                                             # release the B = 256 activations


def test_pgd_linf_through_addnoise_matches_the_fp32_module(model, engines):
    from robustart_amd.model.engine import EngineModel
    from robustart_amd.noise import AddNoise, rng
    torch.manual_seed(6)
    x01 = torch.rand(2, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (2,), device='cuda')
    mean = torch.tensor(MEAN, device='cuda').view(1, 3, 1, 1)
    std = torch.tensor(STD, device='cuda').view(1, 3, 1, 1)
    out = []
    for f_model in (EngineModel(None, takes_normalized=False, engine=engines['fp32x']), lambda z: model((z - mean) / std)):
        rng.manual_seed(11, 0)
        an = AddNoise('pgd_linf')
        an.set_config(f_model=f_model, eps=4 / 255, steps=2)
        out.append(an.add_noise(x01, y))
    xe, xt = out
    same = (xe == xt).double().mean().item()
    with torch.no_grad():
        pe, pt = _fp32_module(model, xe).argmax(1), _fp32_module(model, xt).argmax(1)
        ce = F.cross_entropy(_fp32_module(model, xe), y).item(), F.cross_entropy(_fp32_module(model, x01), y).item()
    print('PGD engine vs module: %.6f of the elements equal; predictions %s / %s; CE clean %.4f -> adversarial %.4f'
          % (same, pe.tolist(), pt.tolist(), ce[1], ce[0]))
    assert (xe - x01).abs().max().item() <= 4 / 255 + 1e-6 and xe.min().item() >= 0 and xe.max().item() <= 1
    assert same >= 0.999 and torch.equal(pe, pt)
    assert ce[0] > ce[1]


def test_solver_evaluate_under_pgd_on_convnextv2():
    from robustart_amd.train import cls_solver as S

    class A:
        engine, corruption, attack, eps, steps, severity, seed, max_iter = 'hip', None, 'pgd_linf', '2/255', 2, 3, 0, 2
    rank, world, device = S.init_dist()
    cfg = {'model': {'type': 'convnextv2_base', 'kwargs': {'num_classes': 1000}},
           'data': {'fake_size': 4, 'batch_size': 4, 'input_size': 224, 'read_from': 'fake'}}
    res = S.evaluate(cfg, A(), rank, world, device)
    assert res['count'] == 4 and res['noise'] == 'pgd_linf' and 0.0 <= res['top1'] <= res['top5'] <= 1.0


def test_attack_entry_never_blocks_the_host(engines):
    from robustart_amd.model.engine import EngineModel
    from robustart_amd.noise import adv
    f = EngineModel(None, takes_normalized=False, engine=engines['bf16'])
    torch.manual_seed(7)
    x = torch.rand(2, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (2,), device='cuda')
    want = adv.pgd_linf(x, y, f, 2 / 255, 3 / 40, 2, seed=9, sample_offset=0)           # warm-up: allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = adv.pgd_linf(x, y, f, 2 / 255, 3 / 40, 2, seed=9, sample_offset=0)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(got, want)
