"""MLP-Mixer-B/16 (model `mixer_b16_224`) without a GPU: the torch module's architecture and timm parameter names, its forward
against an independent fp64 restatement, checkpoint loading, the solver's training guard, the token-mixing GEMM's declaration and
argument checks (csrc/mixer.hip), and the descriptors MixerEngine builds, recorded instead of launched."""
import os
import re

import pytest
import torch
from _recorder import Recorder as _Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['rart_tokmix_bf16', 'rart_tokmix_pair']


def timm_mixer_keys(depth=12):
    keys = ['stem.proj.weight', 'stem.proj.bias']
    for i in range(depth):
        for m in ('norm1', 'mlp_tokens.fc1', 'mlp_tokens.fc2', 'norm2', 'mlp_channels.fc1', 'mlp_channels.fc2'):
            keys += ['blocks.%d.%s.%s' % (i, m, p) for p in ('weight', 'bias')]
    return keys + ['norm.weight', 'norm.bias', 'head.weight', 'head.bias']


def _small(num_classes=10, seed=0):
    """depth 2, 64 channels, 96 px: 36 tokens (not a multiple of 32), token hidden 32, channel hidden 256"""
    from robustart_amd.model.mixer_torch import MlpMixer
    torch.manual_seed(seed)
    m = MlpMixer(num_classes=num_classes, img_size=96, patch_size=16, embed_dim=64, depth=2).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith('bias') or 'norm' in name:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    return m


def test_get_model_builds_mixer_b16_224_with_timm_names():
    from robustart_amd.model import get_model
    m = get_model({'type': 'mixer_b16_224', 'kwargs': {'drop_path': 0.0, 'drop_path_rate': 0.0}})
    sd = m.state_dict()
    assert list(sd.keys()) == timm_mixer_keys()
    assert len(sd) == 150
    assert sum(p.numel() for p in m.parameters()) == 59880472
    b = m.blocks[0]
    assert (b.mlp_tokens.fc1.in_features, b.mlp_tokens.fc1.out_features) == (196, 384)
    assert (b.mlp_channels.fc1.in_features, b.mlp_channels.fc1.out_features) == (768, 3072)
    assert b.norm1.eps == b.norm2.eps == m.norm.eps == 1e-6
    assert m.stem.proj.kernel_size == (16, 16) and m.stem.proj.stride == (16, 16)
    assert get_model({'type': 'mixer_b16_224', 'kwargs': {'num_classes': 10}}).head.out_features == 10


def test_get_model_still_raises_for_other_types():
    from robustart_amd.model import get_model
    with pytest.raises(NotImplementedError, match='MLP-Mixer-B/16'):
        get_model({'type': 'mixer_l16_224'})


def _fp64_forward(m, x):
    """MLP-Mixer written out with einsum in fp64 from the state dict alone"""
    sd = {k: v.double() for k, v in m.state_dict().items()}
    ps = m.patch_size
    x = x.double()
    B, _, H, W = x.shape
    p = x.reshape(B, 3, H // ps, ps, W // ps, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // ps) * (W // ps), 3 * ps * ps)
    t = torch.einsum('bpk,dk->bpd', p, sd['stem.proj.weight'].reshape(sd['stem.proj.weight'].shape[0], -1)) + sd['stem.proj.bias']

    def ln(v, pre):
        mu = v.mean(-1, keepdim=True)
        var = ((v - mu) ** 2).mean(-1, keepdim=True)
        return (v - mu) / torch.sqrt(var + 1e-6) * sd[pre + '.weight'] + sd[pre + '.bias']

    def gelu(v):
        return 0.5 * v * (1 + torch.erf(v / 2 ** 0.5))
    for i in range(len(m.blocks)):
        b = 'blocks.%d.' % i
        y = ln(t, b + 'norm1')
        h = gelu(torch.einsum('jk,bkd->bjd', sd[b + 'mlp_tokens.fc1.weight'], y) + sd[b + 'mlp_tokens.fc1.bias'][:, None])
        t = t + torch.einsum('kj,bjd->bkd', sd[b + 'mlp_tokens.fc2.weight'], h) + sd[b + 'mlp_tokens.fc2.bias'][:, None]
        y = ln(t, b + 'norm2')
        h = gelu(torch.einsum('bkd,hd->bkh', y, sd[b + 'mlp_channels.fc1.weight']) + sd[b + 'mlp_channels.fc1.bias'])
        t = t + torch.einsum('bkh,dh->bkd', h, sd[b + 'mlp_channels.fc2.weight']) + sd[b + 'mlp_channels.fc2.bias']
    pooled = ln(t, 'norm').mean(1)
    return pooled @ sd['head.weight'].t() + sd['head.bias']


def test_reduced_mixer_matches_an_fp64_einsum_restatement():
    m = _small()
    assert m.num_tokens == 36 and m.blocks[0].mlp_tokens.fc1.out_features == 32
    x = torch.rand(3, 3, 96, 96, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        got = m(x).double()
    want = _fp64_forward(m, x)
    assert (got - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())
    # fp64 copy of the module agrees to rounding
    with torch.no_grad():
        assert (m.double()(x.double()) - want).abs().max().item() < 1e-10


def test_drop_path_keys_are_accepted_and_identity_in_eval():
    from robustart_amd.model.mixer_torch import mixer_b16_224
    a = mixer_b16_224(num_classes=10, drop_path=0.1, drop_path_rate=0.1, img_size=64, embed_dim=32, depth=1).eval()
    x = torch.rand(1, 3, 64, 64)
    with torch.no_grad():
        assert torch.equal(a(x), a(x))


def test_timm_checkpoint_loads_strict_and_ignore_model(tmp_path):
    from robustart_amd.train.cls_solver import load_pretrain
    a = _small(num_classes=1000, seed=3)
    sd = a.state_dict()
    path = str(tmp_path / 'mixer.pth')
    torch.save(sd, path)                                          # a bare timm-style state dict
    b = _small(num_classes=1000, seed=4)
    load_pretrain(b, path, strict=True)
    for k, v in sd.items():
        assert torch.equal(v, b.state_dict()[k]), k
    c = _small(num_classes=10, seed=4)
    head = c.head.weight.detach().clone()
    load_pretrain(c, path, strict=True, ignore_model=['head.weight', 'module.head.bias'])
    assert sorted(load_pretrain.last_ignored) == ['head.bias', 'head.weight']
    assert torch.equal(c.head.weight, head) and torch.equal(c.stem.proj.weight, a.stem.proj.weight)
    with pytest.raises(RuntimeError, match='size mismatch'):
        load_pretrain(_small(num_classes=10), path, strict=True)


@pytest.mark.parametrize('engine,train_engine', [('hip', 'hip'), ('torch', 'torch'), ('hip', 'torch')])
def test_training_mixer_fails_loudly(engine, train_engine):
    from robustart_amd.train import cls_solver as S

    class A:
        max_iter = 1
    A.engine, A.train_engine = engine, train_engine
    cfg = {'model': {'type': 'mixer_b16_224', 'kwargs': {'num_classes': 10, 'drop_path': 0.0, 'drop_path_rate': 0.0}},
           'data': {'fake_size': 4, 'batch_size': 2, 'input_size': 224, 'read_from': 'fake'}}
    with pytest.raises(NotImplementedError, match='MLP-Mixer'):
        S.train(cfg, A(), 0, 1, torch.device('cpu'))


def test_make_engine_knows_mixer():
    from robustart_amd.model.engine import make_engine
    if torch.cuda.is_available():
        pytest.skip('GPU present: covered by tests/test_mixer_gpu.py')
    with pytest.raises(RuntimeError, match='no GPU visible'):
        make_engine(_small(), 'cuda')


# ---------------------------------------------------------------------- the C ABI
def test_new_symbols_are_declared_exported_and_bound():
    from robustart_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'robustart_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(rart_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.rart_version() == _lib.ABI_VERSION == 110
    hdr = open(os.path.join(ROOT, 'include', 'robustart_hip.h')).read()
    body = re.search(r'typedef struct rart_tokmix_desc \{(.*?)\} rart_tokmix_desc;', hdr, re.S).group(1)
    fields = re.findall(r'[*\s](\w+)\s*[,;]', body.replace('*', ' '))
    assert fields == [f for f, _ in _lib.TokmixDesc._fields_]


def _desc(**kw):
    from robustart_amd import _lib
    d = _lib.TokmixDesc()
    vals = dict(a_hi=4096, a_lo=8192, x_hi=12288, x_lo=16384, dst_hi=20480, dst_lo=24576, M=384, N=768, K=196, lda=224, ldx=768,
                ldc=768, batch=2, flags=0, x_stride=196 * 768, c_stride=384 * 768)
    vals.update(kw)
    for k, v in vals.items():
        setattr(d, k, v)
    return d


def test_argument_checks_of_the_tokmix_entries_without_gpu():
    """every check happens before a launch, so bad arguments return RART_ERR_INVALID (1) on a GPU-less box"""
    import ctypes
    from robustart_amd import _lib
    lib = _lib.load()

    def err(fn, d, what):
        st = fn(ctypes.byref(d), None)
        assert st == 1, what
        assert what.encode() in lib.rart_last_error_string(), lib.rart_last_error_string()

    bf, pr = lib.rart_tokmix_bf16, lib.rart_tokmix_pair
    err(bf, _desc(lda=200), 'cover K rounded up to 32')
    err(bf, _desc(lda=196), 'cover K rounded up to 32')
    err(bf, _desc(N=764, ldx=764, ldc=764), 'multiples of 8')
    err(bf, _desc(x_stride=195 * 768), "an image's slab")
    err(bf, _desc(c_stride=383 * 768), "an image's slab")
    err(bf, _desc(x_hi=12296), '16-byte aligned')
    err(bf, _desc(flags=4 | 8, aux_hi=4096), 'at most one GELU form')
    err(bf, _desc(flags=64), 'need aux')
    err(bf, _desc(flags=8), 'need aux')
    err(bf, _desc(flags=2 | 64, aux_hi=4096), 'writes bf16')
    err(bf, _desc(flags=16), 'unknown flags')
    err(bf, _desc(batch=0), 'bad sizes')
    err(bf, _desc(batch=70000), 'bad sizes')
    err(pr, _desc(a_lo=None), 'null operand')
    err(pr, _desc(dst_lo=None), 'needs dst_lo')
    err(pr, _desc(res_hi=4096), 'needs res_lo')
    err(pr, _desc(flags=64, aux_hi=4096), 'need aux')
    with pytest.raises(_lib.RartError):
        _lib.check(bf(None, None))


# ---------------------------------------------------------------------- the engine's descriptors, recorded
def _cpu_engine(monkeypatch, model, precision):
    from robustart_amd import _lib
    from robustart_amd.model.engine_base import check_precision
    from robustart_amd.model.mixer_engine import MixerEngine
    monkeypatch.setattr(_lib, 'stream_ptr', lambda: None)
    monkeypatch.setattr(_lib, 'require_gpu', lambda: torch)
    eng = MixerEngine.__new__(MixerEngine)
    eng.lib, eng.profile, eng._buf, eng._w_il = _Recorder(), None, {}, {}
    eng.device, eng.precision = torch.device('cpu'), check_precision(precision)
    eng.D, eng.ps, eng.T = model.embed_dim, model.patch_size, model.num_tokens
    eng.refold(model)
    return eng


def test_token_tables_are_k_padded_with_zero_columns(monkeypatch):
    from robustart_amd.model.mixer_torch import MlpMixer
    m = MlpMixer(num_classes=10, depth=1)                   # B/16 widths: 196 tokens, token hidden 384
    eng = _cpu_engine(monkeypatch, m, 'bf16')
    L = eng.layers[0]
    w1, w2 = m.blocks[0].mlp_tokens.fc1.weight.detach(), m.blocks[0].mlp_tokens.fc2.weight.detach()
    for name, w, shape in (('t1', w1, (384, 224)), ('t2', w2, (196, 384)), ('t1d', w1.t(), (196, 384)), ('t2d', w2.t(), (384, 224))):
        t = L[name]
        assert tuple(t.shape) == shape and t.dtype == torch.bfloat16 and t.is_contiguous(), name
        k = w.shape[1]
        assert torch.equal(t[:, :k], w.to(torch.bfloat16)), name
        assert not t[:, k:].any(), name                      # the zero columns K .. K_pad
    e3 = _cpu_engine(monkeypatch, m, 'fp32x')
    t = e3.layers[0]['t1']
    assert tuple(t.shape) == (2, 384, 224)
    assert (t[0].double() + t[1].double() - torch.nn.functional.pad(w1, (0, 28)).double()).abs().max() <= 2.0 ** -16 * w1.abs().max()
    assert not t[:, :, 196:].any()


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
def test_token_gemm_descriptors(monkeypatch, precision):
    """the four token GEMMs of one block: shared-weight table, K padding (lda 224 for K = 196), per-image strides and the 196-row
    output bound, the epilogue flags"""
    from robustart_amd.model.engine_base import F_GELU, F_GELU_BWD, F_GELU_KEEP
    from robustart_amd.model.mixer_torch import MlpMixer
    m = MlpMixer(num_classes=10, depth=1)
    eng = _cpu_engine(monkeypatch, m, precision)
    x3 = precision == 'fp32x'
    L = eng.layers[0]
    B, T, D, Ht = 3, 196, 768, 384

    def act(*shape):
        return torch.zeros(*(((2,) if x3 else ()) + shape), dtype=torch.bfloat16)
    ln, h, u, xm, x = act(B, T, D), act(B, Ht, D), act(B, Ht, D), act(B, T, D), act(B, T, D)
    eng._tokmix(L['t1'], ln, h, Ht, T, B, bias=L['t1_b'], aux=u, flags=F_GELU_KEEP)
    eng._tokmix(L['t2'], h, xm, T, Ht, B, bias=L['t2_b'], res=x)
    eng._tokmix(L['t2d'], xm, h, Ht, T, B, aux=u, flags=F_GELU_BWD)
    eng._tokmix(L['t1d'], h, ln, T, Ht, B)
    kinds = [k for k, _ in eng.lib.calls]
    assert kinds == ['rart_tokmix_pair' if x3 else 'rart_tokmix_bf16'] * 4
    d = [a[0]._obj for _, a in eng.lib.calls]

    def planes(t):
        return (t[0].data_ptr(), t[1].data_ptr()) if x3 else (t.data_ptr(), None)
    # token fc1: M = 384, K = 196 padded to 224, GELU with u kept
    assert (d[0].M, d[0].N, d[0].K, d[0].lda, d[0].ldx, d[0].ldc, d[0].batch) == (Ht, D, T, 224, D, D, B)
    assert (d[0].x_stride, d[0].c_stride, d[0].flags) == (T * D, Ht * D, F_GELU_KEEP)
    assert (d[0].a_hi, d[0].a_lo) == planes(L['t1']) and (d[0].x_hi, d[0].x_lo) == planes(ln)
    assert (d[0].dst_hi, d[0].dst_lo) == planes(h) and (d[0].aux_hi, d[0].aux_lo) == planes(u)
    assert d[0].bias == L['t1_b'].data_ptr() and d[0].res_hi is None
    # token fc2: the 196-row output bound, + residual
    assert (d[1].M, d[1].K, d[1].lda, d[1].x_stride, d[1].c_stride, d[1].flags) == (T, Ht, Ht, Ht * D, T * D, 0)
    assert (d[1].res_hi, d[1].res_lo) == planes(x) and (d[1].dst_hi, d[1].dst_lo) == planes(xm)
    # dgrad of fc2: W2^T, K padded, GELU'
    assert (d[2].M, d[2].K, d[2].lda, d[2].flags) == (Ht, T, 224, F_GELU_BWD) and (d[2].aux_hi, d[2].aux_lo) == planes(u)
    assert (d[2].a_hi, d[2].a_lo) == planes(L['t2d']) and d[2].bias is None
    # dgrad of fc1: W1^T, no epilogue
    assert (d[3].M, d[3].K, d[3].lda, d[3].flags, d[3].aux_hi, d[3].res_hi) == (T, Ht, Ht, 0, None, None)
    # one table for every image: nothing in the descriptor is per image except the strides
    assert all(c.N == D and c.ldx == D and c.ldc == D for c in d)
    if not x3:
        assert all(c.a_lo is None and c.x_lo is None and c.dst_lo is None for c in d)
    assert F_GELU == 4
