"""rart_expand_walk_pair without a GPU: the engine's switch under the recording library, and the entry's argument checks through the real
library (a refused descriptor never reaches a HIP call)."""
import ctypes

import pytest
import torch

from robustart_amd import _lib
from _recorder import Recorder

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
_MODEL = []


class _Library(Recorder):
    """the recorder with rart_expand_walk_pair_max_k answered by `max_k` (the plain recorder answers 0)"""

    def __init__(self, max_k):
        super().__init__()
        self.max_k = max_k

    def __getattr__(self, name):
        if name == 'rart_expand_walk_pair_max_k':
            return lambda: self.max_k
        return super().__getattr__(name)


def _engine(monkeypatch, rec):
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.noise import adv
    if not _MODEL:
        torch.manual_seed(0)
        _MODEL.append(get_model({'type': 'resnet50_official'}).eval())
    monkeypatch.setattr(_lib, 'require_gpu', lambda: torch)
    monkeypatch.setattr(_lib, 'stream_ptr', lambda: None)
    monkeypatch.setattr(_lib, 'load', lambda: rec)
    monkeypatch.setattr(adv, 'logit_loss', lambda logits, *a: (torch.zeros(2), torch.ones(2, 1000), torch.zeros(2, dtype=torch.int32)))
    eng = ResNet50Engine(_MODEL[0], 'cpu', 'fp32x')
    rec.calls.clear()
    return eng


_FIELDS = ('M', 'N', 'K', 'lda', 'ldw', 'ldc', 'w_rows', 'flags', 'conv', 'batch', 'grid_h', 'grid_w', 'src_h', 'src_w', 'sy', 'sx', 'k_per_tap',
           'n_taps', 'dst_h', 'dst_w', 'dst_sy', 'dst_sx', 'dst_oy', 'dst_ox', 'tile_m', 'tile_n')
_PLANES = ('a_hi', 'a_lo', 'w_hi', 'w_lo', 'bias', 'res_hi', 'res_lo', 'mask_bits', 'sign_out')


def _chain(eng, x):
    """[(entry, what the descriptor of a pair launch says)] of one gradient evaluation.  The weight planes by their addresses, the
    others by whether they are there (gradient buffers may move from one evaluation to the next)"""
    eng.forward_backward(x, MEAN, STD, None, 0)
    out = []
    for n, a in eng.lib.calls:
        d = a[0]._obj if n in ('rart_gemm_pair_bf16', 'rart_expand_walk_pair') else None
        out.append((n, d and tuple(getattr(d, f) for f in _FIELDS) + tuple(getattr(d, f) if f[0] == 'w' else bool(getattr(d, f)) for f in _PLANES)))
    eng.lib.calls.clear()
    return out


def test_query_answering_0_leaves_the_chain_as_it_is(monkeypatch):
    eng = _engine(monkeypatch, Recorder())
    assert eng.expand_walk_max_k == 0
    eng.expand_walk_pair = True
    x = torch.rand(2, 3, 64, 64)
    on = _chain(eng, x)
    eng.expand_walk_pair = False
    off = _chain(eng, x)
    assert on == off and len(on) > 100
    assert not [n for n, _ in on if n == 'rart_expand_walk_pair']


def test_switch_moves_the_identity_launches_of_layer2_and_layer3_only(monkeypatch):
    """with a library that takes K = 256: the expansion and conv1^T of layer2's three and layer3's five identity blocks go to the new
    entry with the very descriptors rart_gemm_pair_bf16 got; nothing else moves"""
    eng = _engine(monkeypatch, _Library(256))
    assert eng.expand_walk_max_k == 256
    eng.expand_walk_pair = True
    x = torch.rand(2, 3, 64, 64)
    on = _chain(eng, x)
    eng.expand_walk_pair = False
    off = _chain(eng, x)
    assert len(on) == len(off)
    moved = [i for i, (a, b) in enumerate(zip(on, off)) if a != b]
    assert len(moved) == 16
    for i in moved:
        assert on[i][0] == 'rart_expand_walk_pair' and off[i][0] == 'rart_gemm_pair_bf16' and on[i][1] == off[i][1]
        d = dict(zip(_FIELDS + _PLANES, on[i][1]))
        assert (d['k_per_tap'], d['N']) in ((128, 512), (256, 1024)) and (d['n_taps'], d['conv']) == (1, 1) and d['res_hi']
        assert not d['tile_m'] and not d['tile_n']
    # a library that takes K = 128 only: layer2's six launches; a width list without 128: layer3's ten
    eng = _engine(monkeypatch, _Library(128))
    eng.expand_walk_pair = True
    assert [n for n, _ in _chain(eng, x)].count('rart_expand_walk_pair') == 6
    eng = _engine(monkeypatch, _Library(256))
    eng.expand_walk_pair, eng.expand_walk_channels = True, (256,)
    assert [n for n, _ in _chain(eng, x)].count('rart_expand_walk_pair') == 10


def _good():
    """a descriptor the entry would launch (fake non-null addresses: the checks never touch them)"""
    d = _lib.GemmPairDesc()
    d.a_hi, d.a_lo, d.w_hi, d.w_lo, d.dst_hi, d.dst_lo = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    d.N, d.lda, d.ldw, d.ldc, d.w_rows = 1024, 256, 768, 1024, 1024
    d.conv, d.batch, d.grid_h, d.grid_w, d.src_h, d.src_w, d.sy, d.sx = 1, 2, 14, 14, 14, 14, 1, 1
    d.k_per_tap, d.n_taps, d.dst_h, d.dst_w, d.dst_sy, d.dst_sx = 256, 1, 14, 14, 1, 1
    return d


@pytest.mark.parametrize('change,message', [
    (lambda d: setattr(d, 'a_lo', None), 'null operand plane'),
    (lambda d: setattr(d, 'dst_lo', None), 'null operand plane'),
    (lambda d: (setattr(d, 'k_per_tap', 512), setattr(d, 'lda', 512), setattr(d, 'ldw', 1536)), 'K must be 128 or 256'),
    (lambda d: setattr(d, 'lda', 260), '16-byte alignment'),
    (lambda d: setattr(d, 'N', 96), 'multiple of 64'),
    (lambda d: setattr(d, 'sy', 2), 'stride 1'),
    (lambda d: setattr(d, 'dst_ox', 1), 'the same pixels'),
    (lambda d: setattr(d, 'flags', 4), 'flags other than ReLU'),
    (lambda d: setattr(d, 'res_hi', 0x7000), 'both planes or none'),
])
def test_refused_arguments(change, message):
    lib = _lib.load()
    assert lib.rart_expand_walk_pair_max_k() == 256
    d = _good()
    change(d)
    assert lib.rart_expand_walk_pair(ctypes.byref(d), 0, 0, None) != 0
    assert message in lib.rart_last_error_string().decode()
    assert lib.rart_expand_walk_pair(None, 0, 0, None) != 0
    assert lib.rart_expand_walk_pair(ctypes.byref(_good()), 96, 0, None) != 0 and 'tile_rows' in lib.rart_last_error_string().decode()
    assert lib.rart_expand_walk_pair(ctypes.byref(_good()), 0, 3, None) != 0 and 'col_parts' in lib.rart_last_error_string().decode()
