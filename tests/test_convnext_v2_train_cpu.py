"""ConvNeXt-V2-B training without a GPU: the GRN parameter-gradient entry of csrc/convnext_v2.hip is declared, exported and bound, its
argument checks run before any launch, its workspace query follows the shape, the closed form it computes matches fp64 autograd
through GlobalResponseNorm, and the train engine refuses stochastic depth before touching the GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['rart_cnx_grn_param_grad_workspace_bytes', 'rart_cnx_grn_bwd_reduce_train_bf16']
EPS = 1e-6


def test_grn_train_symbols_are_declared_exported_and_bound():
    from robustart_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'robustart_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(rart_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.rart_version() == _lib.ABI_VERSION == 110


def test_grn_param_grad_workspace_query():
    from robustart_amd import _lib
    lib = _lib.load()
    for n, c in [(64, 512), (64, 4096), (1, 40), (3, 8)]:
        assert lib.rart_cnx_grn_param_grad_workspace_bytes(n, c) == n * 2 * c * 4, (n, c)
    assert lib.rart_cnx_grn_param_grad_workspace_bytes(2, 44) == 0            # c % 8
    assert lib.rart_cnx_grn_param_grad_workspace_bytes(2, 4104) == 0          # c > 4096
    assert lib.rart_cnx_grn_param_grad_workspace_bytes(0, 512) == 0
    assert lib.rart_cnx_grn_param_grad_workspace_bytes(65536, 512) == 0


def test_argument_checks_of_the_grn_train_entry_without_gpu():
    """every check happens before a launch, so bad arguments return RART_ERR_INVALID (1) on a GPU-less box"""
    from robustart_amd import _lib
    lib = _lib.load()
    p = _lib.c_void_p(4096)                    # never dereferenced: the checks reject the call first
    big = 1 << 30
    f = lib.rart_cnx_grn_bwd_reduce_train_bf16

    def err(st, what):
        assert st == 1, what
        msg = lib.rart_last_error_string()
        assert b'rart_cnx_grn_bwd_reduce_train_bf16' in msg and what.encode() in msg, msg

    for i in range(7):                         # g, y, G, w, a, dw, db
        args = [p] * 7
        args[i] = None
        err(f(*args, 2, 49, 512, EPS, 0, p, big, None), 'bad arguments')
    err(f(p, p, p, p, p, p, p, 2, 49, 512, EPS, 0, None, big, None), 'bad arguments')            # workspace
    err(f(_lib.c_void_p(4104), p, p, p, p, p, p, 2, 49, 512, EPS, 0, p, big, None), 'aligned')   # g
    err(f(p, _lib.c_void_p(4098), p, p, p, p, p, 2, 49, 512, EPS, 0, p, big, None), 'aligned')   # y
    err(f(p, p, p, p, p, p, p, 2, 49, 516, EPS, 0, p, big, None), 'multiple of 8')
    err(f(p, p, p, p, p, p, p, 2, 49, 4104, EPS, 0, p, big, None), 'at most 4096')
    err(f(p, p, p, p, p, p, p, 0, 49, 512, EPS, 0, p, big, None), 'n <= 65535')
    err(f(p, p, p, p, p, p, p, 65536, 49, 512, EPS, 0, p, big, None), 'n <= 65535')
    err(f(p, p, p, p, p, p, p, 2, 0, 512, EPS, 0, p, big, None), 'p > 0')
    err(f(p, p, p, p, p, p, p, 2, 49, 512, EPS, 0, p, 2 * 2 * 512 * 4 - 1, None), 'workspace smaller')
    with pytest.raises(_lib.RartError):
        _lib.check(f(None, None, None, None, None, None, None, 1, 1, 8, EPS, 0, None, 0, None))


def grn_param_grads_closed_form(y, g, w):
    """fp64 dw, db of z = y + b + w * (y * N) over channels-last y, g [n][h][w][c]: dw[c] = sum_n N[n][c] * sum_p g y,
    db[c] = sum_n sum_p g, N = G / (mean_c G + eps), G = ||y[n, :, :, c]||_2 -- what rart_cnx_grn_bwd_reduce_train_bf16 computes"""
    y, g = y.double().flatten(1, 2), g.double().flatten(1, 2)
    G = torch.sqrt((y * y).sum(1))
    N = G / (G.mean(1, keepdim=True) + EPS)
    return (N * (g * y).sum(1)).sum(0), g.sum((0, 1))


@pytest.mark.parametrize('w_kind', ['random', 'zero'])
@pytest.mark.parametrize('zero_channel', [False, True])
def test_grn_param_grad_closed_form_matches_fp64_autograd(w_kind, zero_channel):
    from robustart_amd.model.convnext_torch import GlobalResponseNorm
    gen = torch.Generator().manual_seed(11 + 2 * (w_kind == 'zero') + zero_channel)
    n, h, wd, c = 3, 5, 7, 24
    y = torch.nn.functional.gelu(torch.randn(n, h, wd, c, generator=gen, dtype=torch.float64))
    if zero_channel:
        y[1, :, :, 5] = 0.0                                            # G == 0 for one (image, channel)
    g = torch.randn(n, h, wd, c, generator=gen, dtype=torch.float64)
    m = GlobalResponseNorm(c, eps=EPS).double()
    with torch.no_grad():
        if w_kind == 'random':
            m.weight.copy_(0.5 * torch.randn(c, generator=gen, dtype=torch.float64))
            m.bias.copy_(0.5 * torch.randn(c, generator=gen, dtype=torch.float64))
    m(y).backward(g)
    dw, db = grn_param_grads_closed_form(y, g, m.weight.detach())
    assert torch.isfinite(m.weight.grad).all() and torch.isfinite(dw).all()
    assert torch.allclose(dw, m.weight.grad, rtol=1e-12, atol=1e-12 * dw.abs().max().item())
    assert torch.allclose(db, m.bias.grad, rtol=1e-12, atol=1e-12 * db.abs().max().item())
    # the motivation for the new entry: at w == 0 (timm's init) a = w * sum_p g y is 0, yet dw is not
    assert dw.abs().max() > 0


def test_train_engine_refuses_v2_stochastic_depth_before_touching_the_gpu():
    from robustart_amd.model import get_model
    from robustart_amd.model.convnext_train_engine import ConvNeXtTrainEngine
    m = get_model({'type': 'convnextv2_base', 'kwargs': {'num_classes': 10, 'drop_path_rate': 0.1}})
    with pytest.raises(NotImplementedError, match='drop_path_rate'):
        ConvNeXtTrainEngine(m, 'cuda')
