"""ResNet-18 / ResNet-34 without a GPU: the two types build with the public parameter counts under torchvision's state-dict keys, the
module's forward equals a functional restatement, the bare names still raise, cls_solver refuses to train the types before the model
reaches a device, the entries of csrc/basic_block.hip are declared, exported and bound and check their arguments before any launch, and
the engine's launch plan (driven on the CPU with the library replaced by a recorder) sends exactly the identity blocks of layer1 /
layer2 to rart_basic_block_bf16, once per direction, and none with the switch off, in reference precision or with a projection."""
import ctypes
import os
import re

import pytest
import torch

from _recorder import Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {'resnet18_official': 11689512, 'resnet34_official': 21797672}
LAYERS = {'resnet18_official': (2, 2, 2, 2), 'resnet34_official': (3, 4, 6, 3)}
NEW_SYMBOLS = ['rart_basic_block_supported', 'rart_basic_block_tile', 'rart_basic_block_bf16']
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


@pytest.mark.parametrize('t', sorted(PARAMS))
def test_type_builds_with_the_public_parameter_count_and_torchvisions_keys(t):
    from robustart_amd.model import get_model
    from robustart_amd.model.resnet_basic_torch import BASIC_FAMILY, BasicResNet
    from robustart_amd.model.resnet_torch import ResNet
    m = get_model({'type': t})
    assert isinstance(m, BasicResNet) and not isinstance(m, ResNet) and t in BASIC_FAMILY
    assert sum(p.numel() for p in m.parameters()) == PARAMS[t]
    sd = m.state_dict()
    assert sd['conv1.weight'].shape == (64, 3, 7, 7)
    assert sd['layer1.0.conv1.weight'].shape == (64, 64, 3, 3) and sd['layer2.0.downsample.0.weight'].shape == (128, 64, 1, 1)
    assert sd['layer2.0.conv1.weight'].shape == (128, 64, 3, 3) and sd['layer4.0.conv2.weight'].shape == (512, 512, 3, 3)
    assert sd['fc.weight'].shape == (1000, 512)
    assert not any('conv3' in k or 'bn3' in k for k in sd) and not any(k.startswith('layer1.0.downsample') for k in sd)
    assert [len(getattr(m, 'layer%d' % i)) for i in range(1, 5)] == list(LAYERS[t])
    key = re.compile(r'^(conv1\.weight|bn1\.\w+|fc\.(weight|bias)|layer[1-4]\.\d+\.(conv[12]\.weight|bn[12]\.\w+|downsample\.0\.weight|downsample\.1\.\w+))$')
    assert all(key.match(k) for k in sd), [k for k in sd if not key.match(k)]


def test_kwargs_and_the_names_that_keep_raising():
    from robustart_amd.model import get_model
    m = get_model({'type': 'resnet18_official', 'kwargs': {'num_classes': 10, 'bn': {'use_sync_bn': False}}})
    assert m.fc.out_features == 10 and m.fc.in_features == 512
    for t in ('resnet18', 'resnet34', 'resnet18_v2'):
        with pytest.raises(NotImplementedError, match='outside the hot-path scope') as e:
            get_model({'type': t})
        assert 'MLP-Mixer-B/16' in str(e.value) and 'resnet18_official' in str(e.value)


def test_forward_of_a_tiny_module_matches_a_functional_restatement():
    import torch.nn.functional as F
    from robustart_amd.model.resnet_basic_torch import BasicResNet
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    torch.manual_seed(0)
    layers = (2, 1, 2, 1)
    m = randomize_bn_stats(BasicResNet(layers, num_classes=10)).eval().double()
    sd = m.state_dict()
    x = torch.randn(2, 3, 64, 64, dtype=torch.float64)

    def bn(y, p):
        return F.batch_norm(y, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'], False, 0.0, 1e-5)
    y = F.max_pool2d(F.relu(bn(F.conv2d(x, sd['conv1.weight'], stride=2, padding=3), 'bn1')), 3, 2, 1)
    for li, n in enumerate(layers, 1):
        for b in range(n):
            p = 'layer%d.%d.' % (li, b)
            stride = 2 if (li > 1 and b == 0) else 1
            a = F.relu(bn(F.conv2d(y, sd[p + 'conv1.weight'], stride=stride, padding=1), p + 'bn1'))
            a = bn(F.conv2d(a, sd[p + 'conv2.weight'], padding=1), p + 'bn2')
            if p + 'downsample.0.weight' in sd:
                y = bn(F.conv2d(y, sd[p + 'downsample.0.weight'], stride=stride), p + 'downsample.1')
            y = F.relu(a + y)
    want = F.linear(y.mean((2, 3)), sd['fc.weight'], sd['fc.bias'])
    with torch.no_grad():
        got = m(x)
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('t', sorted(PARAMS))
def test_training_is_refused_before_the_device(t, monkeypatch):
    from robustart_amd.train import cls_solver as S

    def no_device(self, *a, **k):
        raise AssertionError('the model was moved to a device')
    monkeypatch.setattr(torch.nn.Module, 'to', no_device)

    class A:
        max_iter, engine, train_engine = 1, 'hip', 'hip'
    cfg = {'model': {'type': t, 'kwargs': dict(num_classes=10)},
           'data': {'fake_size': 4, 'batch_size': 2, 'input_size': 224, 'read_from': 'fake'}}
    with pytest.raises(NotImplementedError, match='training %r' % t):
        S.train(cfg, A(), 0, 1, torch.device('cuda'))


def test_new_symbols_are_declared_exported_and_bound():
    from robustart_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'robustart_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(rart_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.rart_version() == _lib.ABI_VERSION == 110
    r, c = ctypes.c_int(), ctypes.c_int()
    for ch in (64, 128):
        assert lib.rart_basic_block_tile(ch, ctypes.byref(r), ctypes.byref(c)) == 0 and r.value >= 1 and c.value >= 1
        assert lib.rart_basic_block_supported(ch, 56, 56) == 1 and lib.rart_basic_block_supported(ch, 1, 1) == 1
    assert lib.rart_basic_block_tile(96, ctypes.byref(r), ctypes.byref(c)) == 1
    assert lib.rart_basic_block_supported(96, 56, 56) == 0 and lib.rart_basic_block_supported(64, 0, 56) == 0


def test_argument_checks_of_the_entry_without_gpu():
    """every check happens before a launch, so bad arguments return RART_ERR_INVALID (1) on a GPU-less box"""
    from robustart_amd import _lib
    lib = _lib.load()
    p, odd, n = _lib.c_void_p(4096), _lib.c_void_p(4104), None          # never dereferenced: the checks reject the call first
    taps = (ctypes.c_int * 9)(*[a - 1 for a in range(3) for _ in range(3)])
    tx = (ctypes.c_int * 9)(*[b - 1 for _ in range(3) for b in range(3)])

    def err(st, what):
        assert st == 1, what
        assert what.encode() in lib.rart_last_error_string(), lib.rart_last_error_string()
    # (x, w1, w2, b1, b2, m_mid, m_io, out, n, h, w, channels, tap_dy, tap_dx, backward, stream)
    q = _lib.c_void_p(8192)
    err(lib.rart_basic_block_bf16(n, p, p, p, p, p, p, q, 2, 8, 8, 64, taps, tx, 0, n), 'null tensor')
    err(lib.rart_basic_block_bf16(p, n, p, p, p, p, p, q, 2, 8, 8, 64, taps, tx, 0, n), 'null tensor')
    err(lib.rart_basic_block_bf16(p, p, n, p, p, p, p, q, 2, 8, 8, 64, taps, tx, 0, n), 'null tensor')
    err(lib.rart_basic_block_bf16(p, p, p, p, p, p, p, n, 2, 8, 8, 64, taps, tx, 0, n), 'null tensor')
    err(lib.rart_basic_block_bf16(p, p, p, p, p, p, p, q, 2, 8, 8, 64, None, tx, 0, n), 'null tensor')
    err(lib.rart_basic_block_bf16(p, p, p, n, n, n, p, q, 2, 8, 8, 64, taps, tx, 1, n), 'null tensor')     # the backward needs m_mid
    for ch in (0, 32, 96, 256, 512):
        err(lib.rart_basic_block_bf16(p, p, p, p, p, p, p, q, 2, 8, 8, ch, taps, tx, 0, n), 'unsupported geometry')
    err(lib.rart_basic_block_bf16(p, p, p, p, p, p, p, q, 2, 0, 8, 64, taps, tx, 0, n), 'unsupported geometry')
    err(lib.rart_basic_block_bf16(p, p, p, p, p, p, p, q, 2, 8, -3, 64, taps, tx, 0, n), 'unsupported geometry')
    err(lib.rart_basic_block_bf16(p, p, p, p, p, p, p, q, 0, 8, 8, 64, taps, tx, 0, n), 'n must be positive')
    err(lib.rart_basic_block_bf16(p, p, p, p, p, p, p, q, 1 << 11, 1 << 7, 1 << 7, 64, taps, tx, 0, n), 'below 2^31')
    err(lib.rart_basic_block_bf16(p, p, p, p, p, p, p, p, 2, 8, 8, 64, taps, tx, 0, n), 'alias')
    err(lib.rart_basic_block_bf16(odd, p, p, p, p, p, p, q, 2, 8, 8, 64, taps, tx, 0, n), 'aligned')
    err(lib.rart_basic_block_bf16(p, p, odd, p, p, p, p, q, 2, 8, 8, 64, taps, tx, 0, n), 'aligned')
    err(lib.rart_basic_block_bf16(p, p, p, p, p, p, p, odd, 2, 8, 8, 64, taps, tx, 0, n), 'aligned')
    err(lib.rart_basic_block_bf16(p, p, p, _lib.c_void_p(4098), p, p, p, q, 2, 8, 8, 64, taps, tx, 0, n), 'aligned')
    err(lib.rart_basic_block_bf16(p, p, p, p, p, p, p, q, 2, 8, 8, 64, taps, tx, 2, n), 'backward must be 0 or 1')
    bad = (ctypes.c_int * 9)(*([2] + [0] * 8))
    err(lib.rart_basic_block_bf16(p, p, p, p, p, p, p, q, 2, 8, 8, 64, bad, tx, 0, n), 'taps must lie in -1..1')


# ---------------------------------------------------------------------- launch plan on the CPU
def _engine(monkeypatch, precision, supported=1):
    from robustart_amd import _lib
    from robustart_amd.model.basic_resnet_engine import BasicResNetEngine
    from robustart_amd.model.resnet_basic_torch import BasicResNet
    from robustart_amd.noise import adv
    rec = Recorder()
    rec.supported = lambda name, a: supported if name == 'rart_basic_block_supported' else 0
    monkeypatch.setattr(_lib, 'require_gpu', lambda: torch)
    monkeypatch.setattr(_lib, 'stream_ptr', lambda: None)
    monkeypatch.setattr(_lib, 'load', lambda: rec)
    monkeypatch.setattr(adv, 'logit_loss', lambda logits, *a: (torch.zeros(2), torch.ones(2, 10), torch.zeros(2, dtype=torch.int32)))
    torch.manual_seed(0)
    from robustart_amd.model.basic_resnet_engine import BASIC_BLOCK_SERVED, BASIC_BLOCK_WIDTHS
    eng = BasicResNetEngine(BasicResNet((2, 2, 1, 1), num_classes=10).eval(), 'cpu', precision)
    assert tuple(eng.basic_block_widths) == tuple(BASIC_BLOCK_WIDTHS)          # the default list: the widths that measured faster
    eng.basic_block_widths = BASIC_BLOCK_SERVED                                 # the plan below is the one with every served width listed
    rec.calls.clear()
    return eng, rec


def _fused_calls(eng, rec):
    rec.calls.clear()
    eng.forward_backward(torch.rand(2, 3, 64, 64), MEAN, STD, torch.tensor([1, 2]), 0)
    return [a for n, a in rec.calls if n == 'rart_basic_block_bf16']


def test_launch_plan_one_fused_launch_per_identity_block_and_direction(monkeypatch):
    from robustart_amd.model.basic_resnet_engine import BASIC_BLOCK_SERVED, BASIC_BLOCK_WIDTHS
    eng, rec = _engine(monkeypatch, 'bf16')
    assert eng.basic_block_kernel and BASIC_BLOCK_SERVED == (64, 128) and set(BASIC_BLOCK_WIDTHS) <= set(BASIC_BLOCK_SERVED)
    calls = _fused_calls(eng, rec)
    # (n, h, w, channels, backward): layer1's two identity blocks at 16 x 16 x 64, layer2's second block at 8 x 8 x 128, and back
    plan = [(a[8], a[9], a[10], a[11], a[14]) for a in calls]
    assert plan == [(2, 16, 16, 64, 0), (2, 16, 16, 64, 0), (2, 8, 8, 128, 0), (2, 8, 8, 128, 1), (2, 16, 16, 64, 1), (2, 16, 16, 64, 1)]
    assert all(a[3] is not None and a[4] is not None for a in calls[:3]) and all(a[3] is None and a[4] is None for a in calls[3:])
    assert all(a[5] is not None and a[6] is not None for a in calls)          # both 1-bit tensors in both directions
    n_other = len(rec.calls)
    eng.basic_block_kernel = False
    assert _fused_calls(eng, rec) == [] and len(rec.calls) > n_other           # conv by conv: more launches, none of them fused
    eng.basic_block_kernel, eng.basic_block_widths = True, (128,)
    assert [a[11] for a in _fused_calls(eng, rec)] == [128, 128]
    eng.basic_block_widths = ()
    assert _fused_calls(eng, rec) == []


def test_launch_plan_none_where_the_query_says_no_or_in_reference_precision(monkeypatch):
    eng, rec = _engine(monkeypatch, 'bf16', supported=0)
    assert _fused_calls(eng, rec) == []
    eng, rec = _engine(monkeypatch, 'fp32x')
    assert _fused_calls(eng, rec) == []
    assert any(n == 'rart_gemm_pair_bf16' for n, _ in rec.calls)


def test_inference_forward_issues_the_fused_launch_without_sign_tensors(monkeypatch):
    eng, rec = _engine(monkeypatch, 'bf16')
    eng.logits(torch.rand(2, 3, 64, 64), MEAN, STD)
    calls = [a for n, a in rec.calls if n == 'rart_basic_block_bf16']
    assert len(calls) == 3 and all(a[5] is None and a[6] is None and a[14] == 0 for a in calls)


def test_make_engine_and_refold():
    from robustart_amd.model.basic_resnet_engine import BasicResNetEngine
    from robustart_amd.model.engine import ResNet50Engine, make_engine
    from robustart_amd.model.resnet_basic_torch import BasicResNet
    assert issubclass(BasicResNetEngine, ResNet50Engine)
    m = BasicResNet((1, 1, 1, 1), num_classes=10).eval()
    if torch.cuda.is_available():
        assert isinstance(make_engine(m, 'cuda'), BasicResNetEngine)
    else:            # the dispatch names the engine: the error is the GPU check, not 'no HIP engine'
        with pytest.raises(RuntimeError, match='no GPU visible'):
            make_engine(m, 'cuda')
    bare = object.__new__(BasicResNetEngine)
    bare.precision = 'bf16'
    with pytest.raises(NotImplementedError, match='evaluation only'):
        bare.refold(m)


def test_the_engine_refuses_a_module_outside_its_scope_before_the_gpu():
    from robustart_amd.model.basic_resnet_engine import BasicResNetEngine
    from robustart_amd.model.resnet_basic_torch import BasicResNet
    with pytest.raises(NotImplementedError, match='64 channels'):
        BasicResNetEngine(BasicResNet((1, 1, 1, 1), num_classes=10, width=32).eval(), 'cuda')
