"""MLP-Mixer training without a GPU: the token-mixing gradient entries of csrc/mixer_train.hip (declaration, binding, argument checks),
the rule that splits their contraction over images, the launches MixerTrainEngine.backward records for one block, and the fp64
restatement of the token-parameter gradients (the oracle of tests/test_mixer_train_gpu.py) against torch autograd."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from _recorder import Recorder as _Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['rart_tokmix_wgrad_bf16', 'rart_tok_rowsum_workspace_bytes', 'rart_tok_rowsum_bf16']
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---------------------------------------------------------------------- the oracle
def tok_param_grads_fp64(du_tok, ln1, dxm, h_tok):
    """The four token-parameter gradients written out in fp64 numpy from [B][rows][D] arrays:
    du_tok [B][Ht][D] = (W2^T dx') gelu'(u_tok), ln1 [B][T][D] = LN1(x), dxm [B][T][D] = dx', h_tok [B][Ht][D] = gelu(u_tok)
    -> dW1 [Ht][T], db1 [Ht], dW2 [T][Ht], db2 [T]"""
    du_tok, ln1, dxm, h_tok = (np.asarray(a, dtype=np.float64) for a in (du_tok, ln1, dxm, h_tok))
    dW1 = np.einsum('bhd,btd->ht', du_tok, ln1)
    dW2 = np.einsum('btd,bhd->th', dxm, h_tok)
    return dW1, du_tok.sum((0, 2)), dW2, dxm.sum((0, 2))


def test_fp64_restatement_equals_autograd_through_a_mixer_block():
    from robustart_amd.model.mixer_torch import MixerBlock
    torch.manual_seed(0)
    B, T, D = 3, 20, 24
    blk = MixerBlock(D, T).double()
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.1 * torch.randn_like(p))
    x = torch.randn(B, T, D, dtype=torch.float64)
    mt = blk.mlp_tokens
    # the block's token half with every intermediate a leaf of the graph, [B][rows][D] as the engine stores them
    ln1 = blk.norm1(x)
    u = torch.einsum('ht,btd->bhd', mt.fc1.weight, ln1) + mt.fc1.bias[None, :, None]
    u.retain_grad()
    h = torch.nn.functional.gelu(u)
    xm = x + torch.einsum('th,bhd->btd', mt.fc2.weight, h) + mt.fc2.bias[None, :, None]
    xm.retain_grad()
    out = xm + blk.mlp_channels(blk.norm2(xm))
    assert (out - blk(x)).abs().max().item() < 1e-12                      # the same function as the module
    g = torch.randn(out.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    blk.zero_grad()
    (out * g).sum().backward()
    got = tok_param_grads_fp64(u.grad.numpy(), ln1.detach().numpy(), xm.grad.numpy(), h.detach().numpy())
    want = (mt.fc1.weight.grad, mt.fc1.bias.grad, mt.fc2.weight.grad, mt.fc2.bias.grad)
    for a, b, name in zip(got, want, ('dW1', 'db1', 'dW2', 'db2')):
        b = b.numpy()
        assert a.shape == b.shape, name
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), name


# ---------------------------------------------------------------------- the C ABI
def test_new_symbols_are_declared_exported_and_bound():
    from robustart_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'robustart_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(rart_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.rart_version() == _lib.ABI_VERSION == 110
    body = re.search(r'typedef struct rart_tokmix_wgrad_desc \{(.*?)\} rart_tokmix_wgrad_desc;', hdr, re.S).group(1)
    fields = re.findall(r'[*\s](\w+)\s*[,;]', body.replace('*', ' '))
    assert fields == [f for f, _ in _lib.TokmixWgradDesc._fields_]
    assert ctypes.sizeof(_lib.TokmixWgradDesc) == 3 * 8 + 8 * 4 + 2 * 8


def _desc(**kw):
    from robustart_amd import _lib
    d = _lib.TokmixWgradDesc()
    vals = dict(p=4096, q=8192, partial=12288, M=384, N=196, D=768, batch=8, splits=4, images_per_split=2, ld_partial=384,
                p_stride=384 * 768, q_stride=196 * 768)
    vals.update(kw)
    for k, v in vals.items():
        setattr(d, k, v)
    return d


def test_argument_checks_of_the_token_gradient_entries_without_gpu():
    """every check happens before a launch, so bad arguments return RART_ERR_INVALID (1) on a GPU-less box"""
    from robustart_amd import _lib
    lib = _lib.load()

    def err(st, what):
        assert st == 1, what
        assert what.encode() in lib.rart_last_error_string(), lib.rart_last_error_string()

    wg = lib.rart_tokmix_wgrad_bf16
    err(wg(None, None), 'null descriptor')
    for name in ('p', 'q', 'partial'):
        err(wg(ctypes.byref(_desc(**{name: None})), None), 'null operand')
    err(wg(ctypes.byref(_desc(D=772)), None), 'multiple of 8')
    err(wg(ctypes.byref(_desc(p_stride=384 * 768 - 8)), None), "an image's slab")
    err(wg(ctypes.byref(_desc(q_stride=196 * 768 - 8)), None), "an image's slab")
    err(wg(ctypes.byref(_desc(q_stride=196 * 768 + 4)), None), "an image's slab")
    err(wg(ctypes.byref(_desc(p=4104)), None), '16-byte aligned')
    err(wg(ctypes.byref(_desc(q=8200)), None), '16-byte aligned')
    err(wg(ctypes.byref(_desc(splits=3)), None), 'must cover the batch')
    err(wg(ctypes.byref(_desc(images_per_split=1)), None), 'must cover the batch')
    err(wg(ctypes.byref(_desc(ld_partial=383)), None), 'must cover M')
    for name in ('M', 'N', 'D', 'batch', 'splits', 'images_per_split'):
        err(wg(ctypes.byref(_desc(**{name: 0})), None), 'bad sizes')
    err(wg(ctypes.byref(_desc(splits=70000)), None), 'bad sizes')

    rs = lib.rart_tok_rowsum_bf16
    ok = dict(x=4096, rows=384, dim=768, batch=8, stride=384 * 768, out=8192, accumulate=0, ws=12288, ws_bytes=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        return rs(a['x'], a['rows'], a['dim'], a['batch'], a['stride'], a['out'], a['accumulate'], a['ws'], a['ws_bytes'], None)
    err(call(x=None), 'null operand')
    err(call(out=None), 'null operand')
    err(call(dim=772), 'multiple of 8')
    err(call(stride=384 * 768 - 8), "an image's slab")
    err(call(x=4104), '16-byte aligned')
    for name in ('rows', 'dim', 'batch'):
        err(call(**{name: 0}), 'bad sizes')
    need = lib.rart_tok_rowsum_workspace_bytes(384, 8)
    assert need == 8 * 384 * 4 and lib.rart_tok_rowsum_workspace_bytes(384, 256) == 32 * 384 * 4
    assert lib.rart_tok_rowsum_workspace_bytes(0, 8) == 0
    assert call(ws_bytes=need - 1) == 3 and b'workspace of' in lib.rart_last_error_string()       # RART_ERR_WORKSPACE
    assert call(ws=None) == 3


# ---------------------------------------------------------------------- the split rule
@pytest.mark.parametrize('B', [1, 2, 3, 8, 32, 256, 257])
@pytest.mark.parametrize('M,N', [(384, 196), (196, 384), (40, 24)])
def test_the_split_rule_covers_every_image_once(B, M, N):
    from robustart_amd.model.engine_base import EngineBase, wgrad_split_tokens
    splits, per = wgrad_split_tokens(B, M, N, EngineBase.wgrad_target_wgs)
    assert 1 <= splits <= B and per >= 1
    seen = []
    for z in range(splits):
        rng = list(range(z * per, min(B, (z + 1) * per)))
        assert rng, 'split %d of %d is empty' % (z, splits)
        seen += rng
    assert seen == list(range(B))
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    assert splits * tiles <= max(EngineBase.wgrad_target_wgs, tiles)
    # the library accepts exactly this pair
    assert splits * per >= B


def test_the_split_rule_at_the_training_batch():
    from robustart_amd.model.engine_base import wgrad_split_tokens
    assert wgrad_split_tokens(256, 384, 196, 1024) == (128, 2)            # 6 tiles x 128 splits = 768 workgroups
    assert wgrad_split_tokens(256, 196, 384, 1024) == (128, 2)
    assert wgrad_split_tokens(4, 384, 196, 1024) == (4, 1)


# ---------------------------------------------------------------------- the engine's launches, recorded
def _val(a):
    return a.value if isinstance(a, ctypes.c_void_p) else a


def test_backward_records_the_token_gradient_launches_and_announces_every_parameter(monkeypatch):
    from robustart_amd import _lib
    from robustart_amd.model.engine_base import check_precision
    from robustart_amd.model.mixer_torch import MlpMixer
    from robustart_amd.model.mixer_train_engine import MixerTrainEngine
    monkeypatch.setattr(_lib, 'stream_ptr', lambda: None)
    monkeypatch.setattr(_lib, 'require_gpu', lambda: torch)
    torch.manual_seed(0)
    m = MlpMixer(num_classes=10, depth=1)                   # B/16 widths: 196 tokens, token hidden 384
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    ready = []
    eng = MixerTrainEngine.__new__(MixerTrainEngine)
    eng.lib, eng.profile, eng._buf, eng._w_il = _Recorder(), None, {}, {}
    eng.device, eng.precision = torch.device('cpu'), check_precision('bf16')
    eng.D, eng.ps, eng.T = m.embed_dim, m.patch_size, m.num_tokens
    eng.model, eng.on_grad_ready = m, lambda p: ready.append(id(p))
    eng.refold(m)
    B, T, D, Ht = 2, 196, 768, 384
    logits = eng.forward(torch.rand(B, 3, 224, 224), False, MEAN, STD)
    assert tuple(logits.shape) == (B, 10)
    eng.lib.calls.clear()
    eng.backward(torch.zeros(B, 10))
    params = list(m.parameters())
    assert len(params) == 18
    assert len(ready) == len(set(ready)) == 18 and sorted(ready) == sorted(id(p) for p in params)
    calls = eng.lib.calls
    names = [n for n, _ in calls]
    mt = m.blocks[0].mlp_tokens
    buf = eng._buf
    wg = [i for i, n in enumerate(names) if n == 'rart_tokmix_wgrad_bf16']
    assert len(wg) == 2
    want = [(T, Ht, buf['g_xm'], buf['htok'], mt.fc2.weight), (Ht, T, buf['g_htok'], buf['ln'], mt.fc1.weight)]
    for i, (M, N, p, q, w) in zip(wg, want):
        d = calls[i][1][0]._obj
        assert (d.M, d.N, d.D, d.batch, d.splits, d.images_per_split) == (M, N, D, B, 2, 1)
        assert (d.p_stride, d.q_stride, d.ld_partial) == (M * D, N * D, (M + 7) // 8 * 8)
        assert (d.p, d.q, d.partial) == (p.data_ptr(), q.data_ptr(), buf['tokwg_part'].data_ptr())
        assert buf['tokwg_part'].numel() >= d.splits * N * d.ld_partial * 4
        assert tuple(p.shape) == (B, M, D) and tuple(q.shape) == (B, N, D) and p.dtype == q.dtype == torch.bfloat16
        # the fold that follows: [splits][in = N][ld >= out = M] -> the table's .grad [M][N], written (not accumulated)
        name, a = calls[i + 1]
        assert name == 'rart_wgrad_reduce_f32'
        assert [_val(v) for v in a[:9]] == [d.partial, 2, 1, N, N, M, d.ld_partial, w.grad.data_ptr(), 0]
        assert tuple(w.grad.shape) == (M, N)
    rs = [a for n, a in calls if n == 'rart_tok_rowsum_bf16']
    assert len(rs) == 2
    for a, (M, x, b) in zip(rs, [(T, buf['g_xm'], mt.fc2.bias), (Ht, buf['g_htok'], mt.fc1.bias)]):
        assert [_val(v) for v in a[:7]] == [x.data_ptr(), M, D, B, M * D, b.grad.data_ptr(), 0]
    # gelu(u_tok) is recomputed into the forward's buffer before the fc2 gradient reads it, LN1(x) before the fc1 gradient
    g = [i for i, (n, a) in enumerate(calls) if n == 'rart_gelu_bf16' and _val(a[1]) == buf['htok'].data_ptr()]
    assert len(g) == 1 and g[0] < wg[0]
    ln = [i for i, (n, a) in enumerate(calls) if n == 'rart_layernorm_bf16' and _val(a[0]) == buf['x0'].data_ptr()]
    assert len(ln) == 1 and wg[0] < ln[0] < wg[1]
    # the dgrad chain of MixerEngine.forward_backward is still there: two token GEMMs, in order
    tk = [a[0]._obj for n, a in calls if n == 'rart_tokmix_bf16']
    assert [(t.M, t.K, t.flags) for t in tk] == [(Ht, T, 8), (T, Ht, 0)]


def test_vit_and_mixer_train_engines_share_the_row_helpers():
    from robustart_amd.model.engine_base import RowEngine
    from robustart_amd.model.mixer_train_engine import MixerTrainEngine
    from robustart_amd.model.vit_train_engine import ViTTrainEngine
    for name in ('_ln_bwd_full', '_linear_grads'):
        assert getattr(ViTTrainEngine, name) is getattr(MixerTrainEngine, name) is getattr(RowEngine, name)


def test_model_docstring_and_solver_help_name_the_train_engine():
    import robustart_amd.model as M
    from robustart_amd.train import cls_solver as S
    assert 'MixerTrainEngine' in M.__doc__
    src = open(S.__file__).read()
    assert 'MixerTrainEngine(model, device, on_grad_ready=arena.grad_ready)' in src
