"""ConvNeXt-V2-B (model `convnextv2_base`) without a GPU: the torch module's architecture and timm parameter names, loading the
authors' checkpoint layout, the closed-form GRN backward the kernels implement (fp64, against autograd), the argument checks of the GRN
entries (csrc/convnext_v2.hip) and their declaration / export, and the solver's training guard."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ['rart_cnx_grn_stats_bf16', 'rart_cnx_grn_stats_pair', 'rart_cnx_grn_apply_bf16', 'rart_cnx_grn_apply_pair',
               'rart_cnx_grn_bwd_reduce_bf16', 'rart_cnx_grn_bwd_reduce_pair', 'rart_cnx_grn_bwd_apply_bf16', 'rart_cnx_grn_bwd_apply_pair']


def timm_convnextv2_base_keys():
    keys = ['stem.0.weight', 'stem.0.bias', 'stem.1.weight', 'stem.1.bias']
    for i, depth in enumerate([3, 3, 27, 3]):
        if i > 0:
            keys += ['stages.%d.downsample.%d.%s' % (i, j, p) for j in (0, 1) for p in ('weight', 'bias')]
        for j in range(depth):
            b = 'stages.%d.blocks.%d.' % (i, j)
            keys += [b + m + '.' + p for m in ('conv_dw', 'norm', 'mlp.fc1', 'mlp.grn', 'mlp.fc2') for p in ('weight', 'bias')]
    return keys + ['head.norm.weight', 'head.norm.bias', 'head.fc.weight', 'head.fc.bias']


def _model(**kw):
    from robustart_amd.model import get_model
    return get_model({'type': 'convnextv2_base', 'kwargs': dict({'num_classes': 1000, 'drop_path_rate': 0.1}, **kw)})


def _randomize_grn(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if '.grn.' in name:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
    return m


def to_authors_layout(sd):
    """timm-named state dict -> the ConvNeXt-V2 authors' layout (the inverse of the mapping load_pretrain applies)"""
    out = {}
    for k, v in sd.items():
        m = re.match(r'stem\.(\d)\.(.*)', k)
        if m:
            k = 'downsample_layers.0.%s.%s' % m.groups()
        m = re.match(r'stages\.(\d)\.downsample\.(\d)\.(.*)', k)
        if m:
            k = 'downsample_layers.%s.%s.%s' % m.groups()
        m = re.match(r'stages\.(\d)\.blocks\.(\d+)\.(.*)', k)
        if m:
            i, j, rest = m.groups()
            rest = rest.replace('conv_dw', 'dwconv').replace('mlp.fc1', 'pwconv1').replace('mlp.fc2', 'pwconv2')
            if rest.startswith('mlp.grn.'):
                rest = {'mlp.grn.weight': 'grn.gamma', 'mlp.grn.bias': 'grn.beta'}[rest]
                v = v.reshape(1, 1, 1, -1)
            k = 'stages.%s.%s.%s' % (i, j, rest)
        if k.startswith('head.norm.'):
            k = k[5:]
        elif k.startswith('head.fc.'):
            k = 'head.' + k[8:]
        out[k] = v
    return out


def test_get_model_builds_convnextv2_base_with_timm_names():
    from robustart_amd.model.convnext_torch import ConvNeXt, ConvNeXtV2
    m = _model().eval()
    assert isinstance(m, ConvNeXtV2) and isinstance(m, ConvNeXt) and m.use_grn
    n = sum(p.numel() for p in m.parameters())
    assert n == 88717800, n                                       # timm's convnextv2_base: 88.72 M
    assert list(m.state_dict()) == timm_convnextv2_base_keys()
    assert not any('gamma' in k for k in m.state_dict())
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes['stages.0.blocks.0.mlp.grn.weight'] == (512,)
    assert shapes['stages.3.blocks.2.mlp.grn.bias'] == (4096,)
    assert shapes['stages.2.blocks.26.mlp.fc2.weight'] == (512, 2048)
    assert shapes['head.fc.weight'] == (1000, 1024)
    # timm's init: GRN is the identity
    assert all((v == 0).all() for k, v in m.state_dict().items() if '.grn.' in k)
    with torch.no_grad():
        out = m(torch.rand(1, 3, 64, 64))
    assert out.shape == (1, 1000) and torch.isfinite(out).all()


def test_v1_module_is_unchanged():
    from robustart_amd.model import get_model
    m = get_model({'type': 'convnext_base'})
    assert not getattr(m, 'use_grn', False)
    assert 'stages.0.blocks.0.gamma' in m.state_dict() and not any('grn' in k for k in m.state_dict())


def test_drop_path_is_identity_in_eval():
    m = _randomize_grn(_model(), 0).eval()
    x = torch.rand(2, 3, 32, 32)
    with torch.no_grad():
        assert torch.equal(m(x), m(x))


def test_authors_checkpoint_layout_loads_strict(tmp_path):
    from robustart_amd.train.cls_solver import load_pretrain
    torch.manual_seed(0)
    a = _randomize_grn(_model(depths=(1, 1, 2, 1)), 1).eval()
    sd = a.state_dict()
    off = to_authors_layout(sd)
    assert 'downsample_layers.0.0.weight' in off and 'stages.2.1.pwconv1.weight' in off and 'norm.weight' in off
    assert off['stages.0.0.grn.gamma'].shape == (1, 1, 1, 512) and 'head.weight' in off
    path = str(tmp_path / 'convnextv2_base_1k_224_ema.pt')
    torch.save({'model': off}, path)
    torch.manual_seed(2)
    b = _model(depths=(1, 1, 2, 1)).eval()
    load_pretrain(b, path, strict=True)
    for k, v in sd.items():
        assert torch.equal(v, b.state_dict()[k]), k
    x = torch.rand(2, 3, 64, 64)
    with torch.no_grad():
        assert torch.equal(a(x), b(x))
    # the timm layout still loads as it is
    path2 = str(tmp_path / 'timm.pth')
    torch.save(sd, path2)
    load_pretrain(_model(depths=(1, 1, 2, 1)), path2, strict=True)


@pytest.mark.parametrize('layout', ['authors', 'timm'])
@pytest.mark.parametrize('names', [('head.weight', 'head.bias'), ('head.fc.weight', 'head.fc.bias')])
def test_ignore_model_keys_in_either_layout(tmp_path, layout, names):
    """saver.pretrain.ignore.model: fine-tuning with another class count; the ignored keys may be named in either layout"""
    from robustart_amd.train.cls_solver import load_pretrain
    a = _model(depths=(1, 1, 1, 1), num_classes=1000)
    sd = a.state_dict()
    path = str(tmp_path / 'ck.pt')
    torch.save({'model': to_authors_layout(sd) if layout == 'authors' else sd}, path)
    b = _model(depths=(1, 1, 1, 1), num_classes=10)
    fc = b.head.fc.weight.detach().clone()
    load_pretrain(b, path, strict=True, ignore_model=list(names))
    assert sorted(load_pretrain.last_ignored) == ['head.fc.bias', 'head.fc.weight']
    assert torch.equal(b.head.fc.weight, fc)
    assert torch.equal(b.stem[0].weight, a.stem[0].weight)
    with pytest.raises(KeyError):
        load_pretrain(_model(depths=(1, 1, 1, 1), num_classes=10), path, strict=True, ignore_model=['head.nothing'])


def grn_backward_closed_form(y, u_grad_gelu, g, w, eps=1e-6):
    """the formula the kernels implement (per image, y / g [P][C']): dh = (g (1 + w N) + beta y / G) * GELU'(u)"""
    G = torch.sqrt((y * y).sum(0))
    m = G.mean()
    a = w * (g * y).sum(0)
    s = (a * G).sum()
    C = y.shape[1]
    beta = a / (m + eps) - s / (C * (m + eps) ** 2)
    N = G / (m + eps)
    ratio = torch.where(G > 0, beta / torch.where(G > 0, G, torch.ones_like(G)), torch.zeros_like(G))
    return (g * (1 + w * N) + y * ratio) * u_grad_gelu


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_closed_form_grn_backward_equals_autograd_fp64(seed):
    from robustart_amd.model.convnext_torch import GlobalResponseNorm
    gen = torch.Generator().manual_seed(seed)
    B, H, W, C = 2, 5, 7, 24
    grn = GlobalResponseNorm(C).double()
    with torch.no_grad():
        grn.weight.copy_(0.5 * torch.randn(C, generator=gen, dtype=torch.float64))
        grn.bias.copy_(0.5 * torch.randn(C, generator=gen, dtype=torch.float64))
    u = torch.randn(B, H, W, C, generator=gen, dtype=torch.float64)
    u[1, :, :, 3] = -40.0                          # GELU(-40) == 0 exactly: channel 3 of image 1 has G == 0
    u.requires_grad_(True)
    y = torch.nn.functional.gelu(u)
    z = grn(y)
    gz = torch.randn(B, H, W, C, generator=gen, dtype=torch.float64)
    want, = torch.autograd.grad((z * gz).sum(), u)
    assert (y[1, :, :, 3] == 0).all()
    ud = u.detach()
    gelu_grad = 0.5 * (1 + torch.erf(ud / 2 ** 0.5)) + ud * torch.exp(-ud * ud / 2) / (2 * torch.pi) ** 0.5
    for n in range(B):
        got = grn_backward_closed_form(y[n].detach().reshape(-1, C), gelu_grad[n].reshape(-1, C), gz[n].reshape(-1, C), grn.weight.detach())
        err = (got - want[n].reshape(-1, C)).abs().max().item()
        assert err <= 1e-12 * want.abs().max().item(), err
    # forward formula of the kernels: z = y (1 + w N) + b
    yd = y.detach()
    G = yd.norm(dim=(1, 2), keepdim=True)
    N = G / (G.mean(-1, keepdim=True) + 1e-6)
    torch.testing.assert_close(yd * (1 + grn.weight * N) + grn.bias, z.detach(), rtol=0, atol=1e-13)


def test_new_symbols_are_declared_exported_and_bound():
    from robustart_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'robustart_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(rart_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.rart_version() == _lib.ABI_VERSION == 110


def test_argument_checks_of_the_grn_entries_without_gpu():
    """every check happens before a launch, so bad arguments return RART_ERR_INVALID (1) on a GPU-less box"""
    from robustart_amd import _lib
    lib = _lib.load()
    p, q, r, t = (_lib.c_void_p(v) for v in (4096, 8192, 12288, 16384))      # distinct, 16-byte aligned, never dereferenced

    def err(st, what):
        assert st == 1, what
        assert what.encode() in lib.rart_last_error_string(), lib.rart_last_error_string()

    err(lib.rart_cnx_grn_stats_bf16(None, p, 2, 3136, 512, None), 'rart_cnx_grn_stats_bf16')
    err(lib.rart_cnx_grn_stats_bf16(p, p, 2, 3136, 516, None), 'multiple of 8')
    err(lib.rart_cnx_grn_stats_bf16(p, p, 2, 3136, 16384, None), 'at most 4096')
    err(lib.rart_cnx_grn_stats_bf16(p, p, 0, 3136, 512, None), 'rart_cnx_grn_stats_bf16')
    err(lib.rart_cnx_grn_stats_bf16(p, p, 70000, 49, 512, None), 'n <= 65535')
    err(lib.rart_cnx_grn_stats_bf16(p, p, 2, 0, 512, None), 'p > 0')
    err(lib.rart_cnx_grn_stats_bf16(_lib.c_void_p(4104), p, 2, 49, 512, None), 'aligned')
    err(lib.rart_cnx_grn_stats_pair(p, None, q, 2, 49, 4096, None), 'rart_cnx_grn_stats_pair')
    err(lib.rart_cnx_grn_apply_bf16(p, q, r, None, t, 2, 49, 4096, 1e-6, None), 'rart_cnx_grn_apply_bf16')
    err(lib.rart_cnx_grn_apply_bf16(p, q, r, r, _lib.c_void_p(8200), 2, 49, 4096, 1e-6, None), 'aligned')
    err(lib.rart_cnx_grn_apply_pair(p, q, r, r, r, p, t, 2, 49, 4096, 1e-6, None), 'aliases both planes')   # z_hi == y_hi, z_lo != y_lo
    err(lib.rart_cnx_grn_apply_pair(p, q, r, r, r, t, t, 2, 49, 4100, 1e-6, None), 'multiple of 8')
    err(lib.rart_cnx_grn_bwd_reduce_bf16(p, q, None, r, 2, 49, 4096, None), 'rart_cnx_grn_bwd_reduce_bf16')
    err(lib.rart_cnx_grn_bwd_reduce_pair(p, q, r, t, r, p, 2, 49, 9000, None), 'at most 4096')
    err(lib.rart_cnx_grn_bwd_apply_bf16(p, q, r, t, t, t, q, 2, 49, 4096, 1e-6, None), 'not y or u')      # dh == y
    err(lib.rart_cnx_grn_bwd_apply_bf16(p, q, r, t, t, t, r, 2, 49, 4096, 1e-6, None), 'not y or u')      # dh == u
    err(lib.rart_cnx_grn_bwd_apply_bf16(p, q, r, t, t, t, p, 2, 49, 4100, 1e-6, None), 'multiple of 8')   # dh == g is allowed
    v = [_lib.c_void_p(4096 * k) for k in range(1, 12)]
    err(lib.rart_cnx_grn_bwd_apply_pair(*v[:9], v[0], v[9], 2, 49, 4096, 1e-6, None), 'both planes of g')     # dh_hi == g_hi only
    err(lib.rart_cnx_grn_bwd_apply_pair(*v[:9], v[2], v[3], 2, 49, 4096, 1e-6, None), 'not y or u')           # dh == y
    err(lib.rart_cnx_grn_bwd_apply_pair(*v[:9], v[9], v[10], 2, 0, 4096, 1e-6, None), 'p > 0')
    with pytest.raises(_lib.RartError):
        _lib.check(lib.rart_cnx_grn_stats_pair(None, None, None, 1, 1, 8, None))


@pytest.mark.parametrize('engine,train_engine', [('hip', 'hip'), ('torch', 'torch'), ('hip', 'torch')])
def test_training_convnextv2_fails_loudly(engine, train_engine):
    from robustart_amd.train import cls_solver as S

    class A:
        max_iter = 1
    A.engine, A.train_engine = engine, train_engine
    cfg = {'model': {'type': 'convnextv2_base', 'kwargs': {'num_classes': 10}},
           'data': {'fake_size': 4, 'batch_size': 2, 'input_size': 32, 'read_from': 'fake'}}
    with pytest.raises(NotImplementedError, match='ConvNeXt-V2'):
        S.train(cfg, A(), 0, 1, torch.device('cpu'))


def test_make_engine_knows_convnextv2():
    from robustart_amd.model.engine import make_engine
    if torch.cuda.is_available():
        pytest.skip('GPU present: covered by tests/test_convnext_v2_gpu.py')
    with pytest.raises(RuntimeError, match='no GPU visible'):
        make_engine(_model(), 'cuda')
