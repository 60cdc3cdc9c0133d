"""The streaming attention entries without a GPU: the fp64 reference the GPU tests compare with, the spike inputs of the rescale test,
the C ABI (symbols, signatures, argument checks in front of any HIP call) and the engines' choice between the resident and the
streaming entries, with the library replaced by the recorder."""
import ctypes

import pytest
import torch
from _recorder import Recorder

import _att_stream_ref as R
from robustart_amd import _lib
from robustart_amd.model import engine_base as eb

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ENTRIES = ('rart_vit_attention_stream', 'rart_vit_attention_bwd_stream', 'rart_vit_attention_stream_pair',
           'rart_vit_attention_bwd_stream_pair')


def test_fp64_reference_and_its_autograd_on_the_values_a_pair_represents():
    """attention64 against a per-head loop written out with explicit sums, and its autograd against the closed form of the soft-max
    attention backward; the pair's planes add up to the fp32 input bit for bit"""
    T = 37
    c = R.case(T, 3)
    qs, ds, o64, g64 = c['pair']
    qkv, dout = R.make_inputs(T, 3)
    assert torch.equal((qs[0].float() + qs[1].float()), (qs[0].double() + qs[1].double()).float())
    assert (R.f64(qs) - qkv.double()).abs().max().item() <= 2.0 ** -16 * qkv.abs().max().item()
    q = R.f64(qs).view(R.B, T, 3, R.H, R.HD)
    d = R.f64(ds).view(R.B, T, R.H, R.HD)
    for b in range(R.B):
        for h in range(R.H):
            Q, K, V, dO = q[b, :, 0, h], q[b, :, 1, h], q[b, :, 2, h], d[b, :, h]
            S = Q @ K.T / 8.0
            P = torch.exp(S - S.max(1, keepdim=True).values)
            P = P / P.sum(1, keepdim=True)
            O = P @ V
            assert torch.allclose(o64.view(R.B, T, R.H, R.HD)[b, :, h], O, rtol=0, atol=1e-12)
            dP = dO @ V.T
            dS = P * (dP - (dO * O).sum(1, keepdim=True)) / 8.0
            g = g64.view(R.B, T, 3, R.H, R.HD)[b, :, :, h]
            for got, want in ((g[:, 0], dS @ K), (g[:, 1], dS.T @ Q), (g[:, 2], P.T @ dO)):
                assert torch.allclose(got, want, rtol=0, atol=1e-11)
    qb = c['bf16'][0]
    assert qb.dtype == torch.bfloat16 and torch.equal(qb, R.make_inputs(T, 3, scale=R.SCALE['bf16'])[0].to(torch.bfloat16))


@pytest.mark.parametrize('spike', sorted(R.SPIKES))
def test_spike_inputs_move_the_running_maximum_at_the_chosen_tile(spike):
    """the spiked key's score stands above every other key's for each query of the band -- in the pair's and in the bf16 values -- so
    a kernel that walks the keys raises its running maximum exactly at that key's tile and rescales what it had accumulated (for
    key 0: keeps the first tile's maximum to the end)"""
    T = R.SPIKE_T
    key, q0 = R.SPIKES[spike]
    assert 0 <= key < T and q0 + R.BAND <= T
    c = R.case(T, 900, spike=spike)
    for name in ('pair', 'bf16'):
        qs = c[name][0]
        q64 = R.f64(qs) if name == 'pair' else qs.double()
        ok, margin = R.running_max_moves(q64, T, key, q0)
        assert ok, (name, margin)
        # and the random case does not have it: the check means something
        plain = R.case(T, 900)[name][0]
        assert not R.running_max_moves(R.f64(plain) if name == 'pair' else plain.double(), T, key, q0)[0]
    # the pair format's own error on these inputs leaves the kernel half of the forward bound
    assert R.three_product_forward_error(c['pair'][0], c['pair'][2], T) <= 1.25e-5
    assert {k for k, _ in R.SPIKES.values()} >= {0, T - 1} and any(T // 2 - 32 <= k < T // 2 + 32 for k, _ in R.SPIKES.values())
    assert any(k >= T // 32 * 32 for k, _ in R.SPIKES.values())                  # a key of the last, partial tile


def test_stream_entries_are_exported_with_signatures():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES['rart_vit_attention_stream'] == _lib.SIGNATURES['rart_vit_attention']
    assert _lib.SIGNATURES['rart_vit_attention_stream_pair'] == _lib.SIGNATURES['rart_vit_attention_pair']
    assert _lib.SIGNATURES['rart_vit_attention_bwd_stream_pair'] == _lib.SIGNATURES['rart_vit_attention_bwd_pair']
    res, args = _lib.SIGNATURES['rart_vit_attention_bwd_stream']                  # the resident bf16 backward + stats
    assert len(args) == len(_lib.SIGNATURES['rart_vit_attention_bwd'][1]) + 1 and args[4] == ctypes.c_void_p
    assert _lib.load().rart_version() == _lib.ABI_VERSION == 110                   # additions only


def test_stream_entries_check_their_arguments_before_any_hip_call():
    """status 1 (RART_ERR_INVALID) and a message naming the entry; a HIP call on this path would answer 2 on a machine without a GPU"""
    lib = _lib.load()
    p = ctypes.c_void_p(256)            # never dereferenced: the checks run first
    err = lib.rart_last_error_string

    def fwd(q=p, o=p, T=257, hd=64):
        return lib.rart_vit_attention_stream(q, o, 2, T, 3, hd, None)

    def bwd(q=p, stats=p, T=257, hd=64):
        return lib.rart_vit_attention_bwd_stream(q, p, p, p, stats, 2, T, 3, hd, None)

    def fwd_p(q=p, o=p, T=257, hd=64):
        return lib.rart_vit_attention_stream_pair(p, q, p, o, 2, T, 3, hd, None)

    def bwd_p(q=p, stats=p, T=257, hd=64):
        return lib.rart_vit_attention_bwd_stream_pair(p, q, p, p, p, p, p, p, stats, 2, T, 3, hd, None)

    for name, f in (('rart_vit_attention_stream', fwd), ('rart_vit_attention_bwd_stream', bwd), ('rart_vit_attention_stream_pair', fwd_p),
                    ('rart_vit_attention_bwd_stream_pair', bwd_p)):
        for kw, word in ((dict(q=None), b'bad arguments'), (dict(hd=32), b'head_dim'), (dict(T=0), b'bad arguments'),
                         (dict(T=-5), b'bad arguments'), (dict(T=2 ** 30), b'32-bit')):
            assert f(**kw) == 1, (name, kw)
            assert name.encode() + b':' in err() and word in err(), (name, kw, err())
    assert fwd(o=None) == 1 and fwd_p(o=None) == 1
    for name, f in (('rart_vit_attention_bwd_stream', bwd), ('rart_vit_attention_bwd_stream_pair', bwd_p)):
        assert f(stats=None) == 1 and name.encode() + b':' in err() and b'bad arguments' in err()
    # the resident entries keep their contract
    assert lib.rart_vit_attention(p, p, 2, 225, 3, 64, None) == 1 and b'at most 224 tokens' in err()
    assert lib.rart_vit_attention_bwd_pair(p, p, p, p, p, p, p, p, p, 2, 225, 3, 64, None) == 1 and b'at most 224 tokens' in err()


def _vit(monkeypatch, precision, img):
    """ViTEngine on the CPU with the library replaced by the recorder: patch 16, 2 heads of 64, one block"""
    from robustart_amd.model.vit_engine import ViTEngine
    from robustart_amd.model.vit_torch import VisionTransformer
    torch.manual_seed(0)
    m = VisionTransformer(img_size=img, num_classes=10, embed_dim=128, depth=1, num_heads=2).eval()
    monkeypatch.setattr(_lib, 'require_gpu', lambda: torch)
    monkeypatch.setattr(_lib, 'stream_ptr', lambda: None)
    eng = ViTEngine.__new__(ViTEngine)
    eng.lib, eng.profile, eng._buf, eng._w_il = Recorder(), None, {}, {}
    eng.device, eng.precision = torch.device('cpu'), eb.check_precision(precision)
    eng.D, eng.H, eng.ps, eng.hd, eng.pair_w_interleaved = 128, 2, 16, 64, False
    eng.fused_attention = eng.fused_attention_bwd = True
    eng.refold(m)
    return eng


def _attention_calls(eng, monkeypatch, img, B=2):
    from robustart_amd.noise import adv
    monkeypatch.setattr(adv, 'logit_loss', lambda logits, *a: (torch.zeros(B), torch.ones(B, 10), torch.zeros(B, dtype=torch.int32)))
    eng.lib.calls.clear()
    eng.forward_backward(torch.rand(B, 3, img, img), MEAN, STD, None, 0)
    return [(n, a) for n, a in eng.lib.calls if 'attention' in n or 'softmax' in n]


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
def test_engine_takes_the_stream_entries_above_224_tokens(monkeypatch, precision):
    sfx = '_pair' if precision == 'fp32x' else ''
    eng = _vit(monkeypatch, precision, 256)                                        # 257 tokens
    assert eng.tokens == 257 and eng.stream_attention is None
    calls = _attention_calls(eng, monkeypatch, 256)
    assert [n for n, _ in calls] == ['rart_vit_attention_stream' + sfx, 'rart_vit_attention_bwd_stream' + sfx]
    stats = eng._buf['att_stats']                                                  # both precisions: the backward is two launches
    assert tuple(stats.shape) == (2 * 2, 288, 4) and stats.dtype == torch.float32
    fwd, bwd = calls[0][1], calls[1][1]
    vals = lambda a: [v.value if hasattr(v, 'value') else v for v in a]
    assert vals(fwd)[-5:-1] == [2, 257, 2, 64] and vals(bwd)[-5:-1] == [2, 257, 2, 64]
    assert vals(bwd)[-6] == stats.data_ptr()
    if precision == 'bf16':
        assert tuple(eng._buf['qkv0'].shape) == (2 * 257 + 256, 3 * 128)           # the slack rows stay
    # forced off: the resident entries are asked (and would refuse the shape on the GPU)
    eng.stream_attention = False
    assert [n for n, _ in _attention_calls(eng, monkeypatch, 256)] == ['rart_vit_attention' + sfx, 'rart_vit_attention_bwd' + sfx]


@pytest.mark.parametrize('precision', ['bf16', 'fp32x'])
def test_engine_keeps_the_resident_entries_up_to_224_tokens(monkeypatch, precision):
    sfx = '_pair' if precision == 'fp32x' else ''
    eng = _vit(monkeypatch, precision, 224)                                        # 197 tokens
    assert eng.tokens == 197
    assert [n for n, _ in _attention_calls(eng, monkeypatch, 224)] == ['rart_vit_attention' + sfx, 'rart_vit_attention_bwd' + sfx]
    assert ('att_stats' in eng._buf) == (precision == 'fp32x')                     # bf16: no statistics on the resident route
    eng.stream_attention = True
    assert [n for n, _ in _attention_calls(eng, monkeypatch, 224)] == ['rart_vit_attention_stream' + sfx,
                                                                       'rart_vit_attention_bwd_stream' + sfx]
    assert tuple(eng._buf['att_stats'].shape) == (2 * 2, 224, 4)
    fresh = _vit(monkeypatch, precision, 32)
    assert [fresh._streams(T) for T in (1, 224, 225, 577)] == [False, False, True, True]


def test_unfused_pair_path_refuses_more_than_256_keys_with_a_value_error(monkeypatch):
    eng = _vit(monkeypatch, 'fp32x', 272)                                          # 290 tokens
    eng.fused_attention = False
    with pytest.raises(ValueError, match='256 keys'):
        eng.logits(torch.rand(1, 3, 272, 272), MEAN, STD)
    assert not eng.lib.calls                                                       # refused before the first launch
    eng.fused_attention, eng.fused_attention_bwd = True, False
    with pytest.raises(ValueError, match='256 keys'):
        _attention_calls(eng, monkeypatch, 272, B=1)
    # 225 .. 256 tokens: the unfused path is still there when asked for, and the default is now the fused streaming one
    e256 = _vit(monkeypatch, 'fp32x', 240)                                         # 226 tokens
    assert [n for n, _ in _attention_calls(e256, monkeypatch, 240)] == ['rart_vit_attention_stream_pair', 'rart_vit_attention_bwd_stream_pair']
    e256.fused_attention = e256.fused_attention_bwd = False
    names = [n for n, _ in _attention_calls(e256, monkeypatch, 240)]
    assert 'rart_softmax_rows_pair' in names and not any('attention' in n for n in names)


def test_train_engine_backward_goes_through_the_engines_attention_choice():
    import inspect
    from robustart_amd.model.vit_train_engine import ViTTrainEngine
    src = inspect.getsource(ViTTrainEngine.backward)
    assert 'self._attention_bwd(' in src and 'rart_vit_attention_bwd' not in src
