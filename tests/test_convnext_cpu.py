"""ConvNeXt-B (model `convnext_base`) without a GPU: the torch module's architecture and timm parameter names, checkpoint reload,
the argument checks of the new C-ABI entries (csrc/convnext.hip) and their declaration / export, and the solver's training guard."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ['rart_cnx_dwconv_ln_bf16', 'rart_cnx_dwconv_ln_pair', 'rart_cnx_dwconv_bwd_bf16', 'rart_cnx_dwconv_bwd_pair',
               'rart_cnx_pool_bwd_bf16', 'rart_cnx_pool_bwd_pair', 'rart_cnx_patchify']


def timm_convnext_base_keys():
    """timm's convnext_base state_dict keys, in timm's order: the stem, per stage the downsample (stages 1-3) then per block the layer
    scale, the depthwise conv, the norm and the MLP, then the head."""
    keys = ['stem.0.weight', 'stem.0.bias', 'stem.1.weight', 'stem.1.bias']
    for i, depth in enumerate([3, 3, 27, 3]):
        if i > 0:
            keys += ['stages.%d.downsample.%d.%s' % (i, j, p) for j in (0, 1) for p in ('weight', 'bias')]
        for j in range(depth):
            b = 'stages.%d.blocks.%d.' % (i, j)
            keys += [b + 'gamma'] + [b + m + '.' + p for m in ('conv_dw', 'norm', 'mlp.fc1', 'mlp.fc2') for p in ('weight', 'bias')]
    return keys + ['head.norm.weight', 'head.norm.bias', 'head.fc.weight', 'head.fc.bias']


def _model():
    from robustart_amd.model import get_model
    return get_model({'type': 'convnext_base', 'kwargs': {'num_classes': 1000, 'drop_path_rate': 0.1}})


def test_get_model_builds_convnext_base_with_timm_names():
    m = _model().eval()
    n = sum(p.numel() for p in m.parameters())
    assert 88.5e6 < n < 88.7e6, n                                 # 88 591 464, timm's convnext_base
    assert list(m.state_dict()) == timm_convnext_base_keys()
    assert len(timm_convnext_base_keys()) == 344
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes['stem.0.weight'] == (128, 3, 4, 4)
    assert shapes['stages.1.downsample.1.weight'] == (256, 128, 2, 2)
    assert shapes['stages.2.blocks.26.conv_dw.weight'] == (512, 1, 7, 7)
    assert shapes['stages.3.blocks.2.mlp.fc1.weight'] == (4096, 1024)
    assert shapes['head.fc.weight'] == (1000, 1024)
    with torch.no_grad():
        out = m(torch.rand(1, 3, 64, 64))
    assert out.shape == (1, 1000) and torch.isfinite(out).all()


def test_drop_path_is_identity_in_eval():
    m = _model().eval()
    x = torch.rand(2, 3, 32, 32)
    with torch.no_grad():
        assert torch.equal(m(x), m(x))


def test_state_dict_reloads_strict_through_load_pretrain(tmp_path):
    from robustart_amd.train.cls_solver import load_pretrain
    torch.manual_seed(0)
    a = _model()
    path = str(tmp_path / 'convnext.pth')
    torch.save({'model': {'module.' + k: v for k, v in a.state_dict().items()}}, path)
    torch.manual_seed(1)
    b = _model()
    load_pretrain(b, path, strict=True)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    torch.save(a.state_dict(), path)                              # a bare (timm-style) state dict
    load_pretrain(_model(), path, strict=True)
    _model().load_state_dict(a.state_dict(), strict=True)


def test_new_symbols_are_declared_exported_and_bound():
    from robustart_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'robustart_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(rart_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.rart_version() == _lib.ABI_VERSION == 110


def test_argument_checks_of_the_convnext_entries_without_gpu():
    """every check happens before a launch, so bad arguments return RART_ERR_INVALID (1) on a GPU-less box"""
    from robustart_amd import _lib
    lib = _lib.load()
    p = _lib.c_void_p(16)                      # never dereferenced: the checks reject the call first
    q = _lib.c_void_p(4096)                    # a second, distinct buffer (the outputs that must not alias an input)
    mean = std = (_lib.c_float * 3)(0.5, 0.5, 0.5)

    def err(st, what):
        assert st == 1, what
        assert what.encode() in lib.rart_last_error_string(), lib.rart_last_error_string()

    err(lib.rart_cnx_dwconv_ln_bf16(None, p, p, p, p, p, None, 2, 56, 56, 128, 1e-6, None), 'rart_cnx_dwconv_ln_bf16')
    err(lib.rart_cnx_dwconv_ln_bf16(p, p, p, p, p, q, None, 2, 56, 56, 132, 1e-6, None), 'multiple of 8')     # c % 8
    err(lib.rart_cnx_dwconv_ln_bf16(p, p, p, p, p, q, None, 2, 56, 56, 2048, 1e-6, None), 'at most 1024')
    err(lib.rart_cnx_dwconv_ln_bf16(p, p, p, p, p, q, None, 2, 56, 224, 128, 1e-6, None), 'w * c')         # LDS row
    err(lib.rart_cnx_dwconv_ln_bf16(p, p, p, p, p, _lib.c_void_p(16), None, 2, 56, 56, 128, 1e-6, None), 'bad arguments')  # x == out
    err(lib.rart_cnx_dwconv_ln_pair(p, p, p, p, p, p, _lib.c_void_p(32), _lib.c_void_p(48), p, None, 2, 56, 56, 128, 1e-6, None),
        'bad arguments')                                                                                      # y_hi without y_lo
    err(lib.rart_cnx_dwconv_ln_pair(p, p, p, p, p, p, _lib.c_void_p(32), _lib.c_void_p(48), None, None, 0, 56, 56, 128, 1e-6, None),
        'rart_cnx_dwconv_ln_pair')                                                                            # empty batch
    err(lib.rart_cnx_dwconv_bwd_bf16(p, p, None, p, 2, 56, 56, 128, None), 'must not alias')
    err(lib.rart_cnx_dwconv_ln_bf16(p, _lib.c_void_p(40), p, p, p, q, None, 2, 56, 56, 128, 1e-6, None), 'aligned')     # w_dw
    err(lib.rart_cnx_dwconv_bwd_bf16(_lib.c_void_p(18), p, None, q, 2, 56, 56, 128, None), 'aligned')              # dz
    err(lib.rart_cnx_dwconv_bwd_bf16(p, p, None, _lib.c_void_p(32), 2, 56, 56, 100, None), 'multiple of 8')
    err(lib.rart_cnx_dwconv_bwd_pair(p, None, p, None, None, _lib.c_void_p(32), _lib.c_void_p(48), 2, 7, 7, 1024, None),
        'rart_cnx_dwconv_bwd_pair')
    err(lib.rart_cnx_dwconv_bwd_pair(p, _lib.c_void_p(24), p, p, None, _lib.c_void_p(32), _lib.c_void_p(48), 2, 7, 7, 1024, None),
        'rart_cnx_dwconv_bwd_pair')                                                                           # res_hi without res_lo
    err(lib.rart_cnx_pool_bwd_bf16(p, p, 2, 49, 1020, None), 'rart_cnx_pool_bwd_bf16')
    err(lib.rart_cnx_pool_bwd_pair(p, None, p, p, 2, 49, 1024, None), 'rart_cnx_pool_bwd_pair')
    err(lib.rart_cnx_patchify(p, 0, p, p, 2, 224, 224, 4, 40, mean, std, None), 'row stride')                # ld < 48
    err(lib.rart_cnx_patchify(p, 0, p, p, 2, 224, 224, 4, 60, mean, std, None), 'row stride')                # ld % 8
    err(lib.rart_cnx_patchify(p, 0, p, p, 2, 226, 224, 4, 64, mean, std, None), 'patch side')                # 4 does not divide h
    err(lib.rart_cnx_patchify(p, 1, p, p, 2, 224, 224, 16, 768, mean, std, None), 'patch side')              # > 8
    # rart_vit_patchify keeps its patch % 8 == 0 rule
    err(lib.rart_vit_patchify(p, 0, p, p, 2, 224, 224, 4, mean, std, None), 'multiple of 8')
    with pytest.raises(_lib.RartError):
        _lib.check(lib.rart_cnx_pool_bwd_bf16(None, None, 1, 1, 8, None))


def test_training_convnext_fails_loudly():
    from robustart_amd.train import cls_solver as S

    class A:
        engine, max_iter = 'hip', 1
    cfg = {'model': {'type': 'convnext_base', 'kwargs': {'num_classes': 10}},
           'data': {'fake_size': 4, 'batch_size': 2, 'input_size': 32, 'read_from': 'fake'}}
    with pytest.raises(NotImplementedError, match='no ConvNeXt train engine'):
        S.train(cfg, A(), 0, 1, torch.device('cpu'))


def test_make_engine_knows_convnext():
    """the dispatch names the ConvNeXt engine (building it needs a GPU: the error is the GPU check, not 'no HIP engine')"""
    from robustart_amd.model.engine import make_engine
    m = _model()
    if torch.cuda.is_available():
        pytest.skip('GPU present: covered by tests/test_convnext_gpu.py')
    with pytest.raises(RuntimeError, match='no GPU visible'):
        make_engine(m, 'cuda')
