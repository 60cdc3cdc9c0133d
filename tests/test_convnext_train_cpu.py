"""ConvNeXt-B training without a GPU: the new C-ABI entries of csrc/convnext_train.hip are declared, exported and bound, their argument
checks run before any launch, the workspace queries follow the shape, and the solver's CPU / torch-engine training guard still raises."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ['rart_cnx_dwconv_wgrad_workspace_bytes', 'rart_cnx_dwconv_wgrad_bf16', 'rart_cnx_layer_scale_fwd_bf16',
               'rart_cnx_layer_scale_bwd_workspace_bytes', 'rart_cnx_layer_scale_bwd_bf16']


def test_train_symbols_are_declared_exported_and_bound():
    from robustart_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'robustart_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(rart_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.rart_version() == _lib.ABI_VERSION == 110


def test_workspace_queries():
    from robustart_amd import _lib
    lib = _lib.load()
    for n, h, w, c in [(32, 56, 56, 128), (32, 7, 7, 1024), (1, 7, 9, 40), (3, 13, 17, 8)]:
        got = lib.rart_cnx_dwconv_wgrad_workspace_bytes(n, h, w, c)
        assert got > 0 and got % (50 * 32 * 4) == 0, (n, h, w, c, got)
    assert lib.rart_cnx_dwconv_wgrad_workspace_bytes(2, 56, 56, 132) == 0          # c % 8
    assert lib.rart_cnx_dwconv_wgrad_workspace_bytes(2, 56, 200, 128) == 0         # w > 128
    assert lib.rart_cnx_layer_scale_bwd_workspace_bytes(100352, 128) > 0
    assert lib.rart_cnx_layer_scale_bwd_workspace_bytes(0, 128) == 0
    assert lib.rart_cnx_layer_scale_bwd_workspace_bytes(64, 2048) == 0


def test_argument_checks_of_the_train_entries_without_gpu():
    """every check happens before a launch, so bad arguments return RART_ERR_INVALID (1) on a GPU-less box"""
    from robustart_amd import _lib
    lib = _lib.load()
    p = _lib.c_void_p(16)                      # never dereferenced: the checks reject the call first
    q = _lib.c_void_p(4096)
    big = 1 << 30

    def err(st, what):
        assert st == 1, what
        assert what.encode() in lib.rart_last_error_string(), lib.rart_last_error_string()

    # depthwise weight gradient
    err(lib.rart_cnx_dwconv_wgrad_bf16(None, p, p, p, 2, 56, 56, 128, 0, 0, p, big, None), 'rart_cnx_dwconv_wgrad_bf16')
    err(lib.rart_cnx_dwconv_wgrad_bf16(p, p, None, p, 2, 56, 56, 128, 0, 0, p, big, None), 'bad arguments')          # dw
    err(lib.rart_cnx_dwconv_wgrad_bf16(p, p, p, None, 2, 56, 56, 128, 0, 0, p, big, None), 'bad arguments')          # db
    err(lib.rart_cnx_dwconv_wgrad_bf16(p, p, p, p, 2, 56, 56, 128, 0, 0, None, big, None), 'bad arguments')          # workspace
    err(lib.rart_cnx_dwconv_wgrad_bf16(p, p, p, p, 2, 56, 56, 128, 2, 0, p, big, None), 'bad arguments')             # layout
    err(lib.rart_cnx_dwconv_wgrad_bf16(_lib.c_void_p(18), p, p, p, 2, 56, 56, 128, 0, 0, p, big, None), 'aligned')
    err(lib.rart_cnx_dwconv_wgrad_bf16(p, p, p, p, 2, 56, 56, 132, 0, 0, p, big, None), 'multiple of 8')
    err(lib.rart_cnx_dwconv_wgrad_bf16(p, p, p, p, 2, 7, 7, 2048, 0, 0, p, big, None), 'at most 1024')
    err(lib.rart_cnx_dwconv_wgrad_bf16(p, p, p, p, 2, 56, 200, 128, 0, 0, p, big, None), 'w <=')
    err(lib.rart_cnx_dwconv_wgrad_bf16(p, p, p, p, 0, 56, 56, 128, 0, 0, p, big, None), 'rart_cnx_dwconv_wgrad_bf16')
    err(lib.rart_cnx_dwconv_wgrad_bf16(p, p, p, p, 2, 56, 56, 128, 0, 0, p, 64, None), 'workspace smaller')
    # layer scale
    err(lib.rart_cnx_layer_scale_fwd_bf16(None, p, p, q, 64, 128, None), 'rart_cnx_layer_scale_fwd_bf16')
    err(lib.rart_cnx_layer_scale_fwd_bf16(p, q, p, q, 64, 128, None), 'must not alias u2')
    err(lib.rart_cnx_layer_scale_fwd_bf16(p, q, p, _lib.c_void_p(8200), 64, 128, None), 'aligned')
    err(lib.rart_cnx_layer_scale_fwd_bf16(p, q, p, p, 64, 100, None), 'multiple of 8')
    err(lib.rart_cnx_layer_scale_fwd_bf16(p, q, p, p, 0, 128, None), 'rows')
    err(lib.rart_cnx_layer_scale_bwd_bf16(p, q, p, p, p, None, 64, 128, 0, p, big, None), 'must not alias')         # dv == dx
    err(lib.rart_cnx_layer_scale_bwd_bf16(p, q, p, _lib.c_void_p(8192), None, None, 64, 128, 0, p, big, None), 'bad arguments')
    err(lib.rart_cnx_layer_scale_bwd_bf16(p, q, p, _lib.c_void_p(8200), p, None, 64, 128, 0, p, big, None), 'aligned')
    err(lib.rart_cnx_layer_scale_bwd_bf16(p, q, p, _lib.c_void_p(8192), p, None, 64, 2048, 0, p, big, None), 'at most 1024')
    err(lib.rart_cnx_layer_scale_bwd_bf16(p, q, p, _lib.c_void_p(8192), p, None, 100000, 128, 0, p, 16, None), 'workspace smaller')
    with pytest.raises(_lib.RartError):
        _lib.check(lib.rart_cnx_layer_scale_fwd_bf16(None, None, None, None, 1, 8, None))


def _cfg():
    return {'model': {'type': 'convnext_base', 'kwargs': {'num_classes': 10}},
            'data': {'fake_size': 4, 'batch_size': 2, 'input_size': 32, 'read_from': 'fake'}}


@pytest.mark.parametrize('engine,train_engine', [('hip', 'torch'), ('torch', 'hip')])
def test_training_convnext_off_the_hip_train_engine_fails_loudly(engine, train_engine):
    from robustart_amd.train import cls_solver as S

    class A:
        max_iter = 1
    A.engine, A.train_engine = engine, train_engine
    with pytest.raises(NotImplementedError, match='no ConvNeXt train engine'):
        S.train(_cfg(), A(), 0, 1, torch.device('cpu'))


def test_train_engine_refuses_stochastic_depth_before_touching_the_gpu():
    from robustart_amd.model import get_model
    from robustart_amd.model.convnext_train_engine import ConvNeXtTrainEngine
    m = get_model({'type': 'convnext_base', 'kwargs': {'num_classes': 10, 'drop_path_rate': 0.1}})
    with pytest.raises(NotImplementedError, match='drop_path_rate'):
        ConvNeXtTrainEngine(m, 'cuda')
