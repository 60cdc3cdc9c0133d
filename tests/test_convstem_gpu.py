"""The ConvStem variants of ConvNeXt-B and ViT-B/16 (`convnext_base_cvst`, `vit_base_cvst`) on the HIP engines: the kernels of
csrc/convstem.hip against fp64 torch computations of the same ops, the stem chain (robustart_amd/model/convstem_engine.py) alone against
fp64 on the module's weights, then both whole networks in both precisions, batch invariance of the chain and PGD through AddNoise.

Tolerances stated here:
  * im2col: 2e-5 of max|want| (the hi + lo split of an fp32 value, as the patchify test); col2im: 1e-6 of max|want| (an fp32 sum of at
    most four terms times 1 / std);
  * LayerNorm-GELU kernels vs fp64 of the same (bf16 / pair) operands, the rule of tests/test_convnext_gpu.py: bf16 outputs within
    2^-8 relative + 1e-4 of the scale, pair outputs within 2^-15 relative + 2e-5 of the scale;
  * stem chain vs fp64 on the module's fp32 weights: relative L2 <= 2e-5 (pairs), <= 1e-2 (bf16), the bounds of the downsample test;
  * whole network: the assertions of the ConvNeXt / ViT suites: fp32x logits within 1e-4 of max|logit| of the fp32 module AND of an
    fp64 copy, input gradient relative L2 <= 2e-4 per image, equal predictions, u8 entry within 2e-5 of the scale; bf16 logits within
    2e-2 of the scale, gradient cosine >= 0.999 and relative L2 <= 5e-2;
  * PGD: ||x_adv - x||_inf <= eps + 2^-23 (x_adv is the fp32 rounding of a value inside the ball, values in [0, 1]).
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MODELS = ['convnext_base_cvst', 'vit_base_cvst']


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
    return (t[0].data_ptr(), t[1].data_ptr()) if pair else (t.data_ptr(), None)


def _close(got, ref, pair, what):
    scale = ref.abs().max().item()
    rtol, atol = (2.0 ** -15, 2e-5 * scale) if pair else (2.0 ** -8, 1e-4 * scale)
    err = (got - ref).abs()
    bad = (err > rtol * ref.abs() + atol).sum().item()
    print('%s: max |err| %.3e (scale %.3e), %d outside' % (what, err.max().item(), scale, bad))
    assert bad == 0, what


def _norm64(x01):
    mean = torch.tensor(MEAN, dtype=torch.float64, device=x01.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float64, device=x01.device).view(1, 3, 1, 1)
    return (x01.double() - mean) / std


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('shape', [(2, 24, 40), (2, 224, 224)])
def test_im2col_vs_unfold(shape):
    L, lib = _lib()
    B, H, W = shape
    ld, rows = 32, B * (H // 2) * (W // 2)
    g = torch.Generator(device='cuda').manual_seed(H)
    x = torch.rand(B, 3, H, W, device='cuda', generator=g)
    u8 = (x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    meanf, stdf = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    k = torch.arange(27, device='cuda')
    for src, is_u8, x01 in ((x, 0, x), (u8, 1, u8.permute(0, 3, 1, 2).double() / 255)):
        out = torch.full((2, rows, ld), 7.0, device='cuda').to(torch.bfloat16)              # the padding must be written
        L.check(lib.rart_cvst_im2col(src.data_ptr(), is_u8, out[0].data_ptr(), out[1].data_ptr(), B, H, W, ld, meanf, stdf, L.stream_ptr()))
        want = F.unfold(_norm64(x01), 3, padding=1, stride=2).permute(0, 2, 1).reshape(rows, 27)
        got = _val(out, True)
        assert (got[:, 27:] == 0).all()
        err = (got[:, :27] - want).abs().max().item()
        print('im2col %s u8=%d: max |err| %.2e' % (shape, is_u8, err))
        assert err <= 2e-5 * want.abs().max().item()
        # taps outside the image are 0 in normalised space: the first patch row reads y = -1 at ky = 0, the first column x = -1 at kx = 0
        g4 = got.reshape(B, H // 2, W // 2, ld)
        assert (g4[:, 0][..., :27][..., (k // 3) % 3 == 0] == 0).all() and (g4[:, :, 0][..., :27][..., k % 3 == 0] == 0).all()
        hi_only = torch.full((rows, ld), 7.0, device='cuda').to(torch.bfloat16)              # the lo plane is optional
        L.check(lib.rart_cvst_im2col(src.data_ptr(), is_u8, hi_only.data_ptr(), None, B, H, W, ld, meanf, stdf, L.stream_ptr()))
        assert torch.equal(hi_only, out[0])
    assert lib.rart_cvst_im2col(x.data_ptr(), 0, out[0].data_ptr(), out[1].data_ptr(), B, H - 1, W, ld, meanf, stdf, L.stream_ptr()) == 2


@pytest.mark.parametrize('shape', [(2, 24, 40), (2, 224, 224), (1, 6, 10)])
def test_col2im_vs_fold_and_deterministic(shape):
    """(1, 6, 10): a width that is no multiple of 4 takes the 8-byte store form"""
    L, lib = _lib()
    B, H, W = shape
    ld, P = 32, (H // 2) * (W // 2)
    g = torch.Generator(device='cuda').manual_seed(W)
    dp = torch.randn(B * P, ld, device='cuda', generator=g)
    stdf = (ctypes.c_float * 3)(*STD)
    outs = []
    for _ in range(2):
        grad = torch.full((B, 3, H, W), float('nan'), device='cuda')
        L.check(lib.rart_cvst_col2im_f32(dp.data_ptr(), grad.data_ptr(), B, H, W, ld, stdf, L.stream_ptr()))
        outs.append(grad)
    std = torch.tensor(STD, dtype=torch.float64, device='cuda').view(1, 3, 1, 1)
    want = F.fold(dp[:, :27].double().reshape(B, P, 27).permute(0, 2, 1), (H, W), 3, padding=1, stride=2) / std
    err = (outs[0].double() - want).abs().max().item()
    print('col2im %s: max |err| %.2e' % (shape, err))
    assert torch.isfinite(outs[0]).all() and err <= 1e-6 * want.abs().max().item()
    assert torch.equal(outs[0], outs[1])
    assert lib.rart_cvst_col2im_f32(dp.data_ptr(), grad.data_ptr(), B, H - 1, W, ld, stdf, L.stream_ptr()) == 2


LD = {48: 64, 64: 64, 96: 128, 384: 512, 528: 528}


@pytest.mark.parametrize('pair', [False, True])
@pytest.mark.parametrize('rows', [5, 4097])
@pytest.mark.parametrize('dim', [48, 64, 96, 384, 528])
def test_ln_gelu_forward_and_backward_vs_fp64(dim, rows, pair):
    """5 rows: a partial wave; 4097 rows: a trailing partial block.  Every second row has a large mean (+ 100): a one-pass variance
    would lose it.  Row strides padded (64 for 48, 128 for 96, 512 for 384); the padding columns must come back exactly 0.  528: the
    first width at which a lane holds two 8-channel chunks."""
    L, lib = _lib()
    ld = LD[dim]
    g = torch.Generator(device='cuda').manual_seed(dim + rows)
    x0 = torch.randn(rows, ld, device='cuda', generator=g)
    x0[1::2] += 100.0
    x = _make(x0, pair)
    dy = _make(torch.randn(rows, ld, device='cuda', generator=g), pair)
    gam = (1 + 0.2 * torch.randn(dim, device='cuda', generator=g)).contiguous()
    bet = (0.3 * torch.randn(dim, device='cuda', generator=g)).contiguous()
    out = _make(torch.full((rows, ld), 7.0, device='cuda'), pair)
    dx = _make(torch.full((rows, ld), 7.0, device='cuda'), pair)
    (xh, xl), (yh, yl), (oh, ol), (dh, dl) = _hl(x, pair), _hl(dy, pair), _hl(out, pair), _hl(dx, pair)
    sp = L.stream_ptr()
    if pair:
        L.check(lib.rart_ln_gelu_pair(xh, xl, gam.data_ptr(), bet.data_ptr(), oh, ol, rows, dim, ld, ld, 1e-6, sp))
        L.check(lib.rart_ln_gelu_bwd_pair(yh, yl, xh, xl, gam.data_ptr(), bet.data_ptr(), dh, dl, rows, dim, ld, ld, ld, 1e-6, sp))
    else:
        L.check(lib.rart_ln_gelu_bf16(xh, gam.data_ptr(), bet.data_ptr(), oh, rows, dim, ld, ld, 1e-6, sp))
        L.check(lib.rart_ln_gelu_bwd_bf16(yh, xh, gam.data_ptr(), bet.data_ptr(), dh, rows, dim, ld, ld, ld, 1e-6, sp))
    xr = _val(x, pair)[:, :dim].clone().requires_grad_(True)
    ref = F.gelu(F.layer_norm(xr, (dim,), gam.double(), bet.double(), 1e-6))
    want_dx, = torch.autograd.grad((ref * _val(dy, pair)[:, :dim]).sum(), xr)
    tag = 'dim %d rows %d %s' % (dim, rows, 'pair' if pair else 'bf16')
    got, got_dx = _val(out, pair), _val(dx, pair)
    assert (got[:, dim:] == 0).all() and (got_dx[:, dim:] == 0).all()
    _close(got[:, :dim], ref.detach(), pair, 'ln_gelu ' + tag)
    _close(got_dx[:, :dim], want_dx, pair, 'ln_gelu backward ' + tag)


# ---------------------------------------------------------------------------------------------------------------- engines
def _randomize(m, seed):
    """weights of trained-network magnitude as tests/test_convnext_gpu.py does: layer scales 0.2-0.8, LayerNorm affines near 1 / 0
    (the stem's LayerNorms are `stem.{1,4,7,10}`), depthwise taps 0.1, biases 0.02"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            stem_norm = '.stem.' in name and p.dim() == 1 and int(name.split('.')[-2]) % 3 == 1
            if name.endswith('gamma'):
                p.copy_(0.2 + 0.6 * torch.rand(p.shape, generator=g))
            elif p.dim() == 1 and ('norm' in name or stem_norm or 'downsample.0' in name):
                p.copy_((1.0 if name.endswith('weight') else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith('conv_dw.weight'):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith('bias'):
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    for p in m.parameters():
        p.requires_grad_(False)
    return m.eval()


@pytest.fixture(scope='module', params=MODELS)
def net(request):
    """(type, module on the GPU, {'bf16': engine, 'fp32x': engine}), one at a time"""
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import make_engine
    torch.manual_seed(0)
    m = _randomize(get_model({'type': request.param, 'kwargs': {'num_classes': 1000}}), 1).cuda()
    engines = {'bf16': make_engine(m, 'cuda', 'bf16'), 'fp32x': make_engine(m, 'cuda', 'fp32x')}
    yield request.param, m, engines
    for e in engines.values():
        e._buf.clear()
    torch.cuda.empty_cache()


def _stem_module(m):
    from robustart_amd.model.convstem_torch import convstem_of
    return convstem_of(m)


def _run_stem(kind, eng, x, gval, grad=None):
    """the engine's stem chain alone on x (fp32 NCHW in [0,1]) -> (output rows [B * P][C] fp64, gradient to the image for the output
    gradient gval [B * P][C]).  ViT: the chain writes / reads the patch rows of the token matrix [B][1 + P][D]."""
    pair = eng.x3
    B = x.shape[0]
    if kind.startswith('convnext'):
        C = eng.dims[0]
        out = _make(torch.full((B * 56 * 56, C), float('nan'), device='cuda'), pair)
        eng.cvst.forward(x, False, MEAN, STD, B, 224, 224, out)
        got = _val(out, pair).clone()
        gimg = eng.cvst.backward(_make(gval, pair), STD, grad=grad)
    else:
        P, T, D = 196, 197, eng.D
        out = _make(torch.zeros(B, T, D, device='cuda'), pair)
        eng.cvst.forward(x, False, MEAN, STD, B, 224, 224, out, rows_per_image=P, dst_rows_per_image=T, dst_row_off=1)
        o = _val(out, pair)
        assert (o[:, 0] == 0).all()                                       # the class-token slot is not the stem's
        got = o[:, 1:].reshape(B * P, D).clone()
        gt = torch.zeros(B, T, D, device='cuda')
        gt[:, 1:] = gval.reshape(B, P, D)
        gt[:, 0] = 3.0                                                    # must not reach the image
        gimg = eng.cvst.backward(_make(gt, pair), STD, grad=grad, rows_per_image=P, src_rows_per_image=T, src_row_off=1)
    return got, gimg


@pytest.mark.parametrize('prec', ['bf16', 'fp32x'])
def test_stem_chain_vs_fp64(net, prec):
    kind, m, engines = net
    eng = engines[prec]
    pair = prec == 'fp32x'
    B = 2
    g = torch.Generator(device='cuda').manual_seed(8)
    x = torch.rand(B, 3, 224, 224, device='cuda', generator=g)
    stem64 = copy.deepcopy(_stem_module(m)).double()
    xr = x.double().requires_grad_(True)
    want = stem64(_norm64(xr))                                              # [B][C][h][w]
    C = want.shape[1]
    want_rows = want.permute(0, 2, 3, 1).reshape(-1, C)
    gval = _val(_make(torch.randn(want_rows.shape, device='cuda', generator=g), pair), pair)
    want_g, = torch.autograd.grad((want_rows * gval).sum(), xr)
    grad = torch.full((B, 3, 224, 224), float('nan'), device='cuda')
    got, gimg = _run_stem(kind, eng, x, gval.float() if not pair else gval, grad=grad)
    assert gimg.data_ptr() == grad.data_ptr()
    rel = ((got - want_rows.detach()).norm() / want_rows.norm()).item()
    relg = ((gimg.double() - want_g).norm() / want_g.norm()).item()
    print('%s stem %s: forward rel L2 %.2e, gradient rel L2 %.2e' % (kind, prec, rel, relg))
    rtol = 2e-5 if pair else 1e-2
    assert torch.isfinite(gimg).all() and rel <= rtol and relg <= rtol


def test_stem_chain_b64_matches_b2_bit_for_bit(net):
    """output and gradient of the chain at B = 64 against all 32 B = 2 slices"""
    kind, m, engines = net
    g = torch.Generator(device='cuda').manual_seed(9)
    x = torch.rand(64, 3, 224, 224, device='cuda', generator=g)
    for name, eng in engines.items():
        P, C = (56 * 56, eng.dims[0]) if kind.startswith('convnext') else (196, eng.D)
        gval = torch.randn(64 * P, C, device='cuda', generator=g)
        big, gbig = _run_stem(kind, eng, x, gval)
        gbig = gbig.clone()
        for i in range(0, 64, 2):
            small, gsmall = _run_stem(kind, eng, x[i:i + 2].contiguous(), gval[i * P:(i + 2) * P].contiguous())
            assert torch.equal(small, big[i * P:(i + 2) * P]), (name, i)
            assert torch.equal(gsmall, gbig[i:i + 2]), (name, i)
        eng._buf.clear()


def _fp64_logits_and_grad(model, x, dl):
    m64 = copy.deepcopy(model).cpu().double()
    xr = x.cpu().double().requires_grad_(True)
    lg = m64(_norm64(xr))
    g, = torch.autograd.grad((lg * dl.cpu().double()).sum(), xr)
    return lg.detach().cuda(), g.cuda()


def _fp32_module(model, x):
    mean = torch.tensor(MEAN, device='cuda').view(1, 3, 1, 1)
    std = torch.tensor(STD, device='cuda').view(1, 3, 1, 1)
    return model((x - mean) / std)


def test_fp32x_engine_vs_fp32_module_and_fp64(net):
    kind, model, engines = net
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
    t32 = (pure - ref).abs().max().item()
    a, b = grad.double().flatten(1), want.flatten(1)
    rel = ((a - b).norm(dim=1) / b.norm(dim=1)).cpu()
    xt = x.clone().requires_grad_(True)
    gt, = torch.autograd.grad((_fp32_module(model, xt) * dl).sum(), xt)
    rel_t = ((gt.double().flatten(1) - b).norm(dim=1) / b.norm(dim=1)).cpu()
    print('%s fp32x: max|logit| %.4f; |engine - fp32 module| %.3e (%.2e of scale), |engine - fp64| %.3e (%.2e), '
          '|fp32 module - fp64| %.3e; input gradient rel L2 vs fp64 %s (|grad| %s), torch fp32 autograd %s'
          % (kind, scale, e32, e32 / scale, e64, e64 / scale, t32, rel.tolist(), b.norm(dim=1).tolist(), rel_t.tolist()))
    assert e32 <= 1e-4 * scale and e64 <= 1e-4 * scale
    assert (rel <= 2e-4).all()
    assert torch.equal(pred.long(), ref.argmax(1))
    # the uint8 entry
    u8 = (x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    a8 = eng.logits_from_u8(u8, MEAN, STD)
    b8 = eng.logits(u8.permute(0, 3, 1, 2).float() / 255, MEAN, STD)
    assert (a8 - b8).abs().max().item() <= 2e-5 * scale


def test_bf16_engine_vs_fp32_module(net):
    kind, model, engines = net
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
    print('%s bf16: max|logit| %.4f, |engine - fp32 module| %.3e (%.2e of scale); gradient cos %s, rel L2 %s'
          % (kind, scale, err, err / scale, cos.tolist(), rel.tolist()))
    assert err <= 2e-2 * scale
    assert (cos >= 0.999).all() and (rel <= 5e-2).all()


def test_pgd_linf_through_addnoise_matches_the_fp32_module(net):
    """the same attack (same random start: the process-wide counter reset) through EngineModel(fp32x engine), with the host forbidden to
    wait for the device, and through the fp32 torch module with autograd: the predictions on the adversarial examples agree"""
    from robustart_amd.model.engine import EngineModel
    from robustart_amd.noise import AddNoise, rng
    kind, model, engines = net
    torch.manual_seed(6)
    eps = 2 / 255
    x01 = torch.rand(4, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (4,), device='cuda')
    mean = torch.tensor(MEAN, device='cuda').view(1, 3, 1, 1)
    std = torch.tensor(STD, device='cuda').view(1, 3, 1, 1)

    def attack(f_model):
        rng.manual_seed(11, 0)
        an = AddNoise('pgd_linf')
        an.set_config(f_model=f_model, eps=eps, steps=3)
        return an.add_noise(x01, y)
    f_eng = EngineModel(None, takes_normalized=False, engine=engines['fp32x'])
    attack(f_eng)                                                              # warm-up: allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        xe = attack(f_eng)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    xt = attack(lambda z: model((z - mean) / std))
    with torch.no_grad():
        pe, pt = _fp32_module(model, xe).argmax(1), _fp32_module(model, xt).argmax(1)
    same = (xe == xt).double().mean().item()
    print('%s PGD engine vs module: %.6f of the elements equal; predictions %s / %s' % (kind, same, pe.tolist(), pt.tolist()))
    assert (xe.double() - x01.double()).abs().max().item() <= eps + 2.0 ** -23 and xe.min().item() >= 0 and xe.max().item() <= 1
    assert torch.equal(pe, pt)


def test_solver_evaluate_under_pgd(net):
    from robustart_amd.train import cls_solver as S
    kind = net[0]

    class A:
        engine, corruption, attack, eps, steps, severity, seed, max_iter = 'hip', None, 'pgd_linf', '2/255', 2, 3, 0, 2
    rank, world, device = S.init_dist()
    cfg = {'model': {'type': kind, 'kwargs': {'num_classes': 1000}},
           'data': {'fake_size': 4, 'batch_size': 4, 'input_size': 224, 'read_from': 'fake'}}
    res = S.evaluate(cfg, A(), rank, world, device)
    assert res['count'] == 4 and res['noise'] == 'pgd_linf' and 0.0 <= res['top1'] <= res['top5'] <= 1.0
