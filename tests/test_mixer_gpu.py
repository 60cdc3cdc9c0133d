"""MLP-Mixer-B/16 (model `mixer_b16_224`) on the HIP engine: the token-mixing GEMM of csrc/mixer.hip against fp64 of the same operands
(the block's four shapes and an odd one, batches 1 / 3 / 64, every epilogue flag, the residual aliasing dst), slack rows full of NaN /
inf that must never be read, then MixerEngine in both precisions against the fp32 module and an fp64 copy, batch invariance at B = 256
and run-to-run identity, PGD through AddNoise / EngineModel under torch.cuda.set_sync_debug_mode('error'), and the solver's attacked
evaluation.

Tolerances:
  * kernel, bf16: within one bf16 ulp of the fp64 result of the same bf16 operands, plus the fp32 accumulation slack
    (2 K 2^-24 sum_k |a x|); GELU forms against fp64 of the stored pre-activation u;
  * kernel, pair: per element within (2^-18 + 2 K 2^-24) sum_k |a x| (the lo.lo products left out, fp32 accumulation) + 2^-16 of the
    value (the output's hi / lo split), and within 2e-5 of the output's scale overall;
  * fp32x engine: logits within 1e-4 of max|logit| of the fp32 module and of an fp64 copy; input gradient within 5e-5 relative L2
    of fp64 autograd;
  * bf16 engine: logits within 1e-2 of max|logit| of the fp32 module, input gradient cosine >= 0.999.
"""
import copy
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
F_OUT_F32, F_GELU, F_GELU_BWD, F_GELU_KEEP = 2, 4, 8, 64
SHAPES = [(384, 196, 768), (196, 384, 768), (40, 36, 64)]


def _split(t):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


def _val(t, pair):
    return (t[0].double() + t[1].double()) if pair else t.double()


def _gelu64(v):
    return 0.5 * v * (1 + torch.erf(v / math.sqrt(2)))


def _gelu_grad64(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def _ulp_bf16(v):
    """one bf16 ulp at |v| (2^(e - 7) for 2^e <= |v| < 2^(e+1)); tiny values: the smallest normal's"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def _launch(pair, a, x, dst, M, N, K, B, x_stride, c_stride, ldx=None, ldc=None, bias=None, res=None, aux=None, flags=0):
    from robustart_amd import _lib
    from robustart_amd.model.engine_base import tokmix_desc
    d = tokmix_desc(a, x, dst, M, N, K, B, x_stride, c_stride, ldx=ldx, ldc=ldc, bias=bias, res=res, aux=aux, flags=flags, pair=pair)
    lib = _lib.load()
    _lib.check((lib.rart_tokmix_pair if pair else lib.rart_tokmix_bf16)(ctypes.byref(d), _lib.stream_ptr()))


def _operands(M, K, N, B, pair, seed):
    g = torch.Generator().manual_seed(seed)
    kp = (K + 31) // 32 * 32
    a = torch.zeros(M, kp)
    a[:, :K] = torch.randn(M, K, generator=g) / math.sqrt(K)
    x = torch.randn(B, K, N, generator=g)
    res = torch.randn(B, M, N, generator=g)
    u = torch.randn(B, M, N, generator=g)
    bias = 0.1 * torch.randn(M, generator=g)
    cv = (lambda t: _split(t.cuda())) if pair else (lambda t: t.cuda().to(torch.bfloat16).contiguous())
    return cv(a), cv(x), cv(res), cv(u), bias.cuda()


@pytest.mark.parametrize('pair', [False, True], ids=['bf16', 'pair'])
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%dx%d' % s for s in SHAPES])
def test_token_gemm_vs_fp64(shape, pair):
    M, K, N = shape
    for B in (1, 3, 64):
        a, x, res, u, bias = _operands(M, K, N, B, pair, seed=M + K + B)
        A, X, R, U = _val(a, pair)[:, :K], _val(x, pair), _val(res, pair), _val(u, pair)
        prod = torch.einsum('mk,bkn->bmn', A, X)
        mag = torch.einsum('mk,bkn->bmn', A.abs(), X.abs())
        slack = (2 * K * 2.0 ** -24) * mag
        # pair: three products leave out lo.lo (<= 2^-18 |a x| per term), fp32 accumulation, the hi / lo split of the output
        pslack = (2.0 ** -18 + 2 * K * 2.0 ** -24) * mag
        v = prod + bias.double()[:, None]
        shp = ((2,) if pair else ()) + (B, M, N)

        def new():
            return torch.empty(shp, dtype=torch.bfloat16, device='cuda')

        def check(got, want, extra, what):
            g = _val(got, pair)
            if pair:
                tol = pslack + 2.0 ** -16 * (want.abs() + R.abs()) + 1e-30 + extra
            else:
                tol = _ulp_bf16(want) + slack + extra
            err = (g - want).abs()
            assert torch.isfinite(g).all() and (err <= tol).all(), (what, B, err.max().item(), (err / tol).max().item())
            if pair:        # a few 1e-6 of the output's scale (the lo.lo products left out dominate)
                assert err.max().item() <= 2e-5 * want.abs().max().item(), (what, B, err.max().item() / want.abs().max().item())
        # plain + bias
        out = new()
        _launch(pair, a, x, out, M, N, K, B, K * N, M * N, bias=bias)
        check(out, v, 0, 'bias')
        # no bias, fp32 output
        o32 = torch.empty(B, M, N, device='cuda')
        _launch(pair, a, x, o32, M, N, K, B, K * N, M * N, flags=F_OUT_F32)
        err = (o32.double() - prod).abs()
        assert (err <= (pslack if pair else slack) + 1e-30).all(), ('fp32 out', B, err.max().item())
        # residual aliasing dst
        acc = res.clone()
        _launch(pair, a, x, acc, M, N, K, B, K * N, M * N, bias=bias, res=acc)
        check(acc, v + R, 0, 'residual in place')
        # GELU with u kept, then GELU alone: the same dst bits
        keep_u, keep_h, h = new(), new(), new()
        _launch(pair, a, x, keep_h, M, N, K, B, K * N, M * N, bias=bias, aux=keep_u, flags=F_GELU_KEEP)
        check(keep_u, v, 0, 'kept u')
        ku = _val(keep_u, pair)
        check(keep_h, _gelu64(ku), 5e-7 + 1e-6 * ku.abs(), 'gelu(u)')
        _launch(pair, a, x, h, M, N, K, B, K * N, M * N, bias=bias, flags=F_GELU)
        assert torch.equal(h, keep_h), ('GELU and GELU-keep differ', B)
        # times GELU'(aux)
        gb = new()
        _launch(pair, a, x, gb, M, N, K, B, K * N, M * N, aux=u, flags=F_GELU_BWD)
        gg = _gelu_grad64(U)
        want = prod * gg
        g = _val(gb, pair)
        tol = (pslack * gg.abs() + 2.0 ** -16 * want.abs() + 1e-6 * prod.abs() + 1e-30) if pair else \
            (_ulp_bf16(want) + slack * gg.abs() + 1e-6 * prod.abs())
        err = (g - want).abs()
        assert (err <= tol).all(), ('gelu bwd', B, err.max().item())


@pytest.mark.parametrize('pair', [False, True], ids=['bf16', 'pair'])
def test_slack_rows_and_columns_are_never_read_or_written(pair):
    """slabs with NaN / inf in the rows between and after the images and in the columns past N: the outputs are finite and the same
    bits as a dense run; the destination's slack is left as it was"""
    M, K, N, B = 384, 196, 768, 3             # K = 196: a 32-deep K step reads 28 rows past an image's slab
    a, x, res, u, bias = _operands(M, K, N, B, pair, seed=11)
    ldx, gap = N + 8, 5
    xs = (K + gap) * ldx
    P = (2,) if pair else ()
    big = torch.full(P + (B * xs + 40 * ldx,), float('nan'), dtype=torch.bfloat16, device='cuda')
    big.view(P + (-1,))[..., 1::7] = float('inf')
    big.view(P + (-1,))[..., 2::11] = float('-inf')
    for b in range(B):
        big[..., b * xs: b * xs + K * ldx].view(P + (K, ldx))[..., :N].copy_(x[..., b, :, :] if pair else x[b])
    clean = torch.empty(P + (B, M, N), dtype=torch.bfloat16, device='cuda')
    _launch(pair, a, x, clean, M, N, K, B, K * N, M * N, bias=bias, res=res)
    ldc, cs = N + 16, (M + 3) * (N + 16)
    sentinel = torch.full(P + (B * cs,), 7.0, dtype=torch.bfloat16, device='cuda')
    rs = torch.zeros_like(sentinel)
    for b in range(B):
        rs[..., b * cs: b * cs + M * ldc].view(P + (M, ldc))[..., :N].copy_(res[..., b, :, :] if pair else res[b])
    out = sentinel.clone()
    _launch(pair, a, big, out, M, N, K, B, xs, cs, ldx=ldx, ldc=ldc, bias=bias, res=rs)
    mask = torch.zeros(B * cs, dtype=torch.bool, device='cuda')
    for b in range(B):
        got = out[..., b * cs: b * cs + M * ldc].view(P + (M, ldc))[..., :N]
        want = clean[:, b] if pair else clean[b]
        assert torch.isfinite(got.float()).all() and torch.equal(got, want), b
        mask[b * cs: b * cs + M * ldc].view(M, ldc)[:, :N] = True
    assert torch.equal(out[..., ~mask], sentinel[..., ~mask])


def test_token_gemm_does_not_depend_on_the_batch():
    M, K, N = 384, 196, 768
    for pair in (False, True):
        a, x, res, u, bias = _operands(M, K, N, 64, pair, seed=3)
        full = torch.empty(((2,) if pair else ()) + (64, M, N), dtype=torch.bfloat16, device='cuda')
        _launch(pair, a, x, full, M, N, K, 64, K * N, M * N, bias=bias, flags=F_GELU)
        for i in (0, 37, 63):
            xi = (x[:, i:i + 1] if pair else x[i:i + 1]).contiguous()
            one = torch.empty(((2,) if pair else ()) + (1, M, N), dtype=torch.bfloat16, device='cuda')
            _launch(pair, a, xi, one, M, N, K, 1, K * N, M * N, bias=bias, flags=F_GELU)
            assert torch.equal(one, full[:, i:i + 1] if pair else full[i:i + 1]), (pair, i)


# ---------------------------------------------------------------------- the engine
def _randomize(m, seed):
    """trained-network magnitudes: LayerNorm affines near 1 / 0, small biases"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1 and 'norm' in name:
                p.copy_((1.0 if name.endswith('weight') else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith('bias'):
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    return m.eval()


@pytest.fixture(scope='module')
def model():
    from robustart_amd.model import get_model
    torch.manual_seed(0)
    return _randomize(get_model({'type': 'mixer_b16_224', 'kwargs': {'num_classes': 1000, 'drop_path': 0.0, 'drop_path_rate': 0.0}}),
                      1).cuda()


@pytest.fixture(scope='module')
def engines(model):
    from robustart_amd.model.engine import make_engine
    from robustart_amd.model.mixer_engine import MixerEngine
    e = {'bf16': make_engine(model, 'cuda', 'bf16'), 'fp32x': make_engine(model, 'cuda', 'fp32x')}
    assert all(isinstance(x, MixerEngine) for x in e.values())
    return e


def _fp64_logits_and_grad(model, x, dl):
    m64 = copy.deepcopy(model).double()
    mean = torch.tensor(MEAN, dtype=torch.float64, device='cuda').view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float64, device='cuda').view(1, 3, 1, 1)
    xr = x.double().requires_grad_(True)
    lg = m64((xr - mean) / std)
    g, = torch.autograd.grad((lg * dl.double()).sum(), xr)
    return lg.detach(), g


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
    assert torch.equal(eng.logits(x, MEAN, STD), logits)
    dl = eng.last_dlogits.clone()
    with torch.no_grad():
        pure = _fp32_module(model, x).double()
    ref, want = _fp64_logits_and_grad(model, x, dl)
    scale = ref.abs().max().item()
    e32 = (logits.double() - pure).abs().max().item()
    e64 = (logits.double() - ref).abs().max().item()
    a, b = grad.double().flatten(1), want.flatten(1)
    rel = ((a - b).norm(dim=1) / b.norm(dim=1)).cpu()
    print('Mixer fp32x: max|logit| %.4f; |engine - fp32 module| %.3e (%.2e of scale), |engine - fp64| %.3e (%.2e); '
          'input gradient rel L2 vs fp64 %s' % (scale, e32, e32 / scale, e64, e64 / scale, rel.tolist()))
    assert e32 <= 1e-4 * scale and e64 <= 1e-4 * scale
    assert (rel <= 5e-5).all()
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
    print('Mixer bf16: max|logit| %.4f, |engine - fp32 module| %.3e (%.2e of scale); gradient cos %s'
          % (scale, err, err / scale, cos.tolist()))
    assert err <= 1e-2 * scale
    assert (cos >= 0.999).all()
    f = eng.logits(x, MEAN, STD)
    assert (f - logits).abs().max().item() <= 1e-2 * scale


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
    f_eng = EngineModel(None, takes_normalized=False, engine=engines['fp32x'])
    rng.manual_seed(11, 0)
    an = AddNoise('pgd_linf')
    an.set_config(f_model=f_eng, eps=4 / 255, steps=2)
    an.add_noise(x01, y)                                            # warm-up: allocations
    torch.cuda.synchronize()
    out = []
    for f_model in (f_eng, lambda z: model((z - mean) / std)):
        rng.manual_seed(11, 0)
        an = AddNoise('pgd_linf')
        an.set_config(f_model=f_model, eps=4 / 255, steps=2)
        if f_model is f_eng:
            torch.cuda.set_sync_debug_mode('error')
            try:
                out.append(an.add_noise(x01, y))
            finally:
                torch.cuda.set_sync_debug_mode('default')
        else:
            out.append(an.add_noise(x01, y))
    xe, xt = out
    same = (xe == xt).double().mean().item()
    with torch.no_grad():
        pe, pt = _fp32_module(model, xe).argmax(1), _fp32_module(model, xt).argmax(1)
        ce = F.cross_entropy(_fp32_module(model, xe), y).item(), F.cross_entropy(_fp32_module(model, x01), y).item()
    print('Mixer PGD engine vs module: %.6f of the elements equal; predictions %s / %s; CE clean %.4f -> adversarial %.4f'
          % (same, pe.tolist(), pt.tolist(), ce[1], ce[0]))
    assert (xe - x01).abs().max().item() <= 4 / 255 + 1e-6 and xe.min().item() >= 0 and xe.max().item() <= 1
    assert same >= 0.999 and torch.equal(pe, pt)
    assert ce[0] > ce[1]


def test_solver_evaluate_under_pgd_on_mixer():
    from robustart_amd.train import cls_solver as S

    class A:
        engine, corruption, attack, eps, steps, severity, seed, max_iter = 'hip', None, 'pgd_linf', '2/255', 2, 3, 0, 2
    rank, world, device = S.init_dist()
    cfg = {'model': {'type': 'mixer_b16_224', 'kwargs': {'num_classes': 1000, 'drop_path': 0.0, 'drop_path_rate': 0.0}},
           'data': {'fake_size': 4, 'batch_size': 4, 'input_size': 224, 'read_from': 'fake'}}
    res = S.evaluate(cfg, A(), rank, world, device)
    assert res['count'] == 4 and res['noise'] == 'pgd_linf' and 0.0 <= res['top1'] <= res['top5'] <= 1.0
