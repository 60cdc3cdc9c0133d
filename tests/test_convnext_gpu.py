"""ConvNeXt-B (model `convnext_base`) on the HIP engine: the new kernels of csrc/convnext.hip and the downsample's GEMM scatter
against fp64 torch computations of the same ops, then the whole engine (ConvNeXtEngine, robustart_amd/model/convnext_engine.py) in
both precisions against the fp32 module and an fp64 copy, batch invariance at B = 256, PGD through AddNoise / EngineModel, the
solver's attacked evaluation and the attack entry under torch.cuda.set_sync_debug_mode('error').

Tolerances stated here:
  * kernels vs fp64 of the same (bf16 / pair) operands: bf16 outputs within one bf16 rounding (2^-8 relative) + 1e-4 of the scale;
    pair outputs within 2^-15 relative + 2e-5 of the scale (the fp32 arithmetic and the output split);
  * downsample conv / scatter (GEMMs on the engine's weight tables): relative L2 <= 1e-2 (bf16 weights), <= 2e-5 (pairs);
  * fp32x engine: logits within 1e-4 of max|logit| of the fp32 module AND of an fp64 copy; input gradient vs fp64 autograd:
    relative L2 <= 2e-4 per image (measured 2e-5);
  * bf16 engine vs the fp32 module: logits within 2e-2 of max|logit| (measured 7e-3), input gradient cosine >= 0.999 (measured
    0.9999) and relative L2 <= 5e-2 (measured 1.4e-2).
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
STAGES = [(56, 128), (28, 256), (14, 512), (7, 1024)]          # (side, channels) at 224 x 224


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


def _dw_ref(x, w49, flip=False):
    """fp64 7x7 depthwise correlation (padding 3) of NHWC x with taps w49 [49][C]; flip: the transposed convolution"""
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 3, 3, 3, 3))
    out = torch.zeros_like(x)
    for dy in range(7):
        for dx in range(7):
            t = (6 - dy) * 7 + (6 - dx) if flip else dy * 7 + dx
            out += xp[:, dy:dy + H, dx:dx + W, :] * w49[t]
    return out


def _ln_ref(y, g, b, eps=1e-6):
    mu = y.mean(-1, keepdim=True)
    var = ((y - mu) ** 2).mean(-1, keepdim=True)
    return (y - mu) / torch.sqrt(var + eps) * g + b


def _shapes():
    return [(2, s, s, c) for s, c in STAGES] + [(256, 56, 56, 128)]


def test_transposed_taps_are_the_autograd_of_the_depthwise_conv():
    """the fp64 reference's flip is the input gradient of a grouped conv2d (CPU, fp64)"""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 9, 11, 8, generator=g, dtype=torch.float64)
    w = torch.randn(8, 1, 7, 7, generator=g, dtype=torch.float64)
    dz = torch.randn(2, 9, 11, 8, generator=g, dtype=torch.float64)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    out = F.conv2d(xr, w, padding=3, groups=8)
    want, = torch.autograd.grad((out * dz.permute(0, 3, 1, 2)).sum(), xr)
    w49 = w.reshape(8, 49).t()
    torch.testing.assert_close(_dw_ref(x, w49), out.detach().permute(0, 2, 3, 1))
    torch.testing.assert_close(_dw_ref(dz, w49, flip=True), want.permute(0, 2, 3, 1))


@pytest.mark.parametrize('pair', [False, True])
@pytest.mark.parametrize('shape', _shapes())
def test_dwconv_ln_forward_vs_fp64(shape, pair):
    L, lib = _lib()
    B, H, W, C = shape
    g = torch.Generator(device='cuda').manual_seed(B * 7 + C)
    x = _make(torch.randn(B, H, W, C, device='cuda', generator=g), pair)
    w49 = (0.15 * torch.randn(49, C, device='cuda', generator=g)).contiguous()
    bdw = (0.1 * torch.randn(C, device='cuda', generator=g)).contiguous()
    gam = (1 + 0.2 * torch.randn(C, device='cuda', generator=g)).contiguous()
    bet = (0.1 * torch.randn(C, device='cuda', generator=g)).contiguous()
    out = torch.empty_like(x)
    yk = torch.empty_like(x)
    xh, xl = _hl(x, pair)
    oh, ol = _hl(out, pair)
    yh, yl = _hl(yk, pair)
    sp = L.stream_ptr()
    if pair:
        st = lib.rart_cnx_dwconv_ln_pair(xh, xl, w49.data_ptr(), bdw.data_ptr(), gam.data_ptr(), bet.data_ptr(), oh, ol, yh, yl, B, H, W,
                                         C, 1e-6, sp)
    else:
        st = lib.rart_cnx_dwconv_ln_bf16(xh, w49.data_ptr(), bdw.data_ptr(), gam.data_ptr(), bet.data_ptr(), oh, yh, B, H, W, C, 1e-6, sp)
    L.check(st)
    xv = _val(x, pair)
    del x
    y = _dw_ref(xv, w49.double()) + bdw.double()
    del xv
    _close(_val(yk, pair), y, pair, 'dwconv output %s %s' % (shape, 'pair' if pair else 'bf16'))
    _close(_val(out, pair), _ln_ref(y, gam.double(), bet.double()), pair, 'dwconv+LN %s %s' % (shape, 'pair' if pair else 'bf16'))


@pytest.mark.parametrize('pair', [False, True])
@pytest.mark.parametrize('shape', _shapes())
def test_dwconv_backward_vs_fp64(shape, pair):
    """dx = res + transposed 7x7 of dz, written in place over the residual gradient (the engine's call) and out of place without res"""
    L, lib = _lib()
    B, H, W, C = shape
    g = torch.Generator(device='cuda').manual_seed(B * 11 + C)
    dz = _make(torch.randn(B, H, W, C, device='cuda', generator=g), pair)
    res = _make(torch.randn(B, H, W, C, device='cuda', generator=g), pair)
    w49 = (0.15 * torch.randn(49, C, device='cuda', generator=g)).contiguous()
    want = _dw_ref(_val(dz, pair), w49.double(), flip=True)
    want_res = want + _val(res, pair)
    zh, zl = _hl(dz, pair)
    rh, rl = _hl(res, pair)
    plain = torch.empty_like(dz)
    ph, pl = _hl(plain, pair)
    sp = L.stream_ptr()
    if pair:
        L.check(lib.rart_cnx_dwconv_bwd_pair(zh, zl, w49.data_ptr(), rh, rl, rh, rl, B, H, W, C, sp))
        L.check(lib.rart_cnx_dwconv_bwd_pair(zh, zl, w49.data_ptr(), None, None, ph, pl, B, H, W, C, sp))
    else:
        L.check(lib.rart_cnx_dwconv_bwd_bf16(zh, w49.data_ptr(), rh, rh, B, H, W, C, sp))
        L.check(lib.rart_cnx_dwconv_bwd_bf16(zh, w49.data_ptr(), None, ph, B, H, W, C, sp))
    tag = '%s %s' % (shape, 'pair' if pair else 'bf16')
    _close(_val(res, pair), want_res, pair, 'dwconv backward + residual ' + tag)
    _close(_val(plain, pair), want, pair, 'dwconv backward ' + tag)


@pytest.mark.parametrize('pair', [False, True])
def test_pool_backward(pair):
    L, lib = _lib()
    B, hw, C = 4, 49, 1024
    dp = _make(torch.randn(B, C, device='cuda'), pair)
    dz = _make(torch.empty(B, hw, C, device='cuda'), pair)
    if pair:
        L.check(lib.rart_cnx_pool_bwd_pair(dp[0].data_ptr(), dp[1].data_ptr(), dz[0].data_ptr(), dz[1].data_ptr(), B, hw, C, L.stream_ptr()))
    else:
        L.check(lib.rart_cnx_pool_bwd_bf16(dp.data_ptr(), dz.data_ptr(), B, hw, C, L.stream_ptr()))
    _close(_val(dz, pair), (_val(dp, pair) / hw)[:, None, :].expand(B, hw, C), pair, 'pool backward')


@pytest.mark.parametrize('B', [2, 256])
def test_stem_patchify_and_unpatchify_vs_fp64(B):
    L, lib = _lib()
    g = torch.Generator(device='cuda').manual_seed(B)
    x = torch.rand(B, 3, 224, 224, device='cuda', generator=g)
    u8 = (x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    P, ld = 56 * 56, 64
    mean, std = torch.tensor(MEAN, dtype=torch.float64, device='cuda'), torch.tensor(STD, dtype=torch.float64, device='cuda')
    meanf, stdf = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    for src, is_u8, x01 in ((x, 0, x.double()), (u8, 1, u8.permute(0, 3, 1, 2).double() / 255)):
        out = torch.full((2, B * P, ld), 7.0, device='cuda').to(torch.bfloat16)        # the padding must be written
        L.check(lib.rart_cnx_patchify(src.data_ptr(), is_u8, out[0].data_ptr(), out[1].data_ptr(), B, 224, 224, 4, ld, meanf, stdf,
                                      L.stream_ptr()))
        xn = (x01 - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)
        want = xn.reshape(B, 3, 56, 4, 56, 4).permute(0, 2, 4, 1, 3, 5).reshape(B * P, 48)
        got = _val(out, True)
        assert (got[:, 48:] == 0).all()
        err = (got[:, :48] - want).abs().max().item()
        print('patchify B=%d u8=%d: max |err| %.2e' % (B, is_u8, err))
        assert err <= 2e-5 * want.abs().max().item()
    dp = torch.randn(B * P, ld, device='cuda')
    grad = torch.empty(B, 3, 224, 224, device='cuda')
    L.check(lib.rart_vit_unpatchify_from_f32(dp.data_ptr(), grad.data_ptr(), B, 224, 224, 4, ld, stdf, L.stream_ptr()))
    want = dp[:, :48].double().reshape(B, 56, 56, 3, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 224, 224) / std.view(1, 3, 1, 1)
    err = (grad.double() - want).abs().max().item()
    print('unpatchify B=%d: max |err| %.2e' % (B, err))
    assert err <= 1e-6 * want.abs().max().item()


# ---------------------------------------------------------------------------------------------------------------- whole network
def _randomize(m, seed):
    """weights of trained-network magnitude: layer scales 0.2-0.8 (the 1e-6 init would hide every block), LayerNorm affines near 1 / 0"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith('gamma'):
                p.copy_(0.2 + 0.6 * torch.rand(p.shape, generator=g))
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
    return _randomize(get_model({'type': 'convnext_base', 'kwargs': {'num_classes': 1000}}), 1).cuda()


@pytest.fixture(scope='module')
def engines(model):
    from robustart_amd.model.engine import make_engine
    return {'bf16': make_engine(model, 'cuda', 'bf16'), 'fp32x': make_engine(model, 'cuda', 'fp32x')}


@pytest.mark.parametrize('prec', ['bf16', 'fp32x'])
@pytest.mark.parametrize('si', [1, 2, 3])
def test_downsample_conv_and_scatter_vs_fp64(model, engines, prec, si):
    """the 2x2 stride-2 conv on the GEMM's conv mode (after the LayerNorm) and its backward, four parity GEMMs scattering with
    destination stride 2, against fp64 products on the module's fp32 weights; B = 256 at the stage-1 shape"""
    eng = engines[prec]
    pair = prec == 'fp32x'
    S = eng.stages[si]
    (side, cin), (_, cout) = STAGES[si - 1], STAGES[si]
    conv, ln = model.stages[si].downsample[1], model.stages[si].downsample[0]
    W = conv.weight.detach().double().permute(0, 2, 3, 1).reshape(cout, 4 * cin)       # [cout][(ty, tx, c)]
    rtol = 2e-5 if pair else 1e-2
    for B in ([2, 256] if si == 1 else [2]):
        g = torch.Generator(device='cuda').manual_seed(B + si)
        x = _make(torch.randn(B * side * side, cin, device='cuda', generator=g), pair)
        out = _make(torch.empty(B * (side // 2) ** 2, cout, device='cuda'), pair)
        eng._downsample(x, S, out, B, side, side)
        xl = _ln_ref(_val(x, pair), ln.weight.double(), ln.bias.double()).reshape(B, side // 2, 2, side // 2, 2, cin)
        want = xl.permute(0, 1, 3, 2, 4, 5).reshape(-1, 4 * cin) @ W.t() + conv.bias.double()
        got = _val(out, pair)
        rel = ((got - want).norm() / want.norm()).item()
        dy = _make(torch.randn(B * (side // 2) ** 2, cout, device='cuda', generator=g), pair)
        dx = _make(torch.full((B * side * side, cin), float('nan'), device='cuda'), pair)          # every pixel must be written
        eng._downsample_scatter(dy, S, dx, B, side, side)
        wantd = (_val(dy, pair) @ W).reshape(B, side // 2, side // 2, 2, 2, cin).permute(0, 1, 3, 2, 4, 5).reshape(-1, cin)
        gotd = _val(dx, pair)
        reld = ((gotd - wantd).norm() / wantd.norm()).item()
        print('downsample %s stage %d B=%d: conv rel L2 %.2e, scatter rel L2 %.2e' % (prec, si, B, rel, reld))
        assert torch.isfinite(gotd).all() and rel <= rtol and reld <= rtol


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
    t32 = (pure - ref).abs().max().item()
    a, b = grad.double().flatten(1), want.flatten(1)
    rel = ((a - b).norm(dim=1) / b.norm(dim=1)).cpu()
    xt = x.clone().requires_grad_(True)
    gt, = torch.autograd.grad((_fp32_module(model, xt) * dl).sum(), xt)
    rel_t = ((gt.double().flatten(1) - b).norm(dim=1) / b.norm(dim=1)).cpu()
    print('ConvNeXt fp32x: max|logit| %.4f; |engine - fp32 module| %.3e (%.2e of scale), |engine - fp64| %.3e (%.2e), '
          '|fp32 module - fp64| %.3e; input gradient rel L2 vs fp64 %s (|grad| %s), torch fp32 autograd %s'
          % (scale, e32, e32 / scale, e64, e64 / scale, t32, rel.tolist(), b.norm(dim=1).tolist(), rel_t.tolist()))
    assert e32 <= 1e-4 * scale and e64 <= 1e-4 * scale
    assert (rel <= 2e-4).all()
    assert torch.equal(pred.long(), ref.argmax(1))
    # the uint8 entry
    u8 = (x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    a8 = eng.logits_from_u8(u8, MEAN, STD)
    b8 = eng.logits(u8.permute(0, 3, 1, 2).float() / 255, MEAN, STD)
    assert (a8 - b8).abs().max().item() <= 2e-5 * scale


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
    print('ConvNeXt bf16: max|logit| %.4f, |engine - fp32 module| %.3e (%.2e of scale); gradient cos %s, rel L2 %s'
          % (scale, err, err / scale, cos.tolist(), rel.tolist()))
    assert err <= 2e-2 * scale
    assert (cos >= 0.999).all() and (rel <= 5e-2).all()
    f = eng.logits(x, MEAN, STD)
    assert (f - logits).abs().max().item() <= 1e-2 * scale       # forward-only fc1: GELU of the fp32 pre-activation


def test_engines_b256_match_b8_bit_for_bit(model, engines):
    g = torch.Generator().manual_seed(5)
    x = torch.rand(256, 3, 224, 224, generator=g).cuda()
    y = torch.randint(0, 1000, (256,), generator=g).cuda()
    for name, eng in engines.items():
        big = eng.logits(x, MEAN, STD).clone()
        lb, _, gb, _ = eng.forward_backward(x, MEAN, STD, y, 0)
        lb, gb = lb.clone(), gb.clone()
        for i in (0, 120, 248):
            xs, ys = x[i:i + 8].contiguous(), y[i:i + 8].contiguous()
            assert torch.equal(eng.logits(xs, MEAN, STD), big[i:i + 8]), (name, i)
            ls, _, gs, _ = eng.forward_backward(xs, MEAN, STD, ys, 0)
            assert torch.equal(ls, lb[i:i + 8]) and torch.equal(gs, gb[i:i + 8]), (name, i)
        eng._buf.clear()                                             # release the B = 256 activations


def test_pgd_linf_through_addnoise_matches_the_fp32_module(model, engines):
    """the same attack (same random start: the process-wide counter reset) through EngineModel(fp32x engine) and through the fp32 torch
    module with autograd: the adversarial examples and the predictions on them agree"""
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


def test_solver_evaluate_under_pgd_on_convnext():
    from robustart_amd.train import cls_solver as S

    class A:
        engine, corruption, attack, eps, steps, severity, seed, max_iter = 'hip', None, 'pgd_linf', '2/255', 2, 3, 0, 2
    rank, world, device = S.init_dist()
    cfg = {'model': {'type': 'convnext_base', 'kwargs': {'num_classes': 1000}},
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
