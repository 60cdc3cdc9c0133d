"""DenseNet-121 / -169 / -201 without a GPU: the three types build with the public parameter counts under torchvision's state-dict keys,
the module's forward equals a functional restatement, the entries of csrc/densenet.hip are declared, exported and bound and check their
arguments before any launch, make_engine dispatches to DenseNetEngine, the engine refuses widths that are no multiple of 32 before it
touches a GPU, and cls_solver refuses to train the types before the model reaches a device."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {'densenet121': 7978856, 'densenet169': 14149480, 'densenet201': 20013928}
BLOCKS = {'densenet121': (6, 12, 24, 16), 'densenet169': (6, 12, 32, 32), 'densenet201': (6, 12, 48, 32)}
_BN = r'(weight|bias|running_mean|running_var|num_batches_tracked)'
_KEY = re.compile(r'^(features\.conv0\.weight|features\.norm[05]\.' + _BN + r'|classifier\.(weight|bias)|'
                  r'features\.denseblock[1-4]\.denselayer\d+\.(conv[12]\.weight|norm[12]\.' + _BN + r')|'
                  r'features\.transition[1-3]\.(conv\.weight|norm\.' + _BN + r'))$')
NEW_SYMBOLS = ['rart_dn_%s_%s' % (k, s) for k in ('preact', 'preact_bwd', 'preact_pool2', 'preact_pool2_bwd', 'copy') for s in ('bf16', 'pair')]


@pytest.fixture(scope='module')
def models():
    from robustart_amd.model import get_model
    return {t: get_model({'type': t}) for t in PARAMS}


@pytest.mark.parametrize('t', sorted(PARAMS))
def test_type_builds_with_the_public_parameter_count_and_torchvisions_keys(models, t):
    m = models[t]
    assert sum(p.numel() for p in m.parameters()) == PARAMS[t]
    sd = m.state_dict()
    assert all(_KEY.match(k) for k in sd), [k for k in sd if not _KEY.match(k)]
    assert m.block_config == BLOCKS[t] and m.growth_rate == 32 and m.bn_size == 4
    c = 64
    for i, n in enumerate(BLOCKS[t], 1):
        assert len(getattr(m.features, 'denseblock%d' % i)) == n
        for j in range(1, n + 1):
            p = 'features.denseblock%d.denselayer%d.' % (i, j)
            assert sd[p + 'norm1.weight'].shape == (c + 32 * (j - 1),) and sd[p + 'conv1.weight'].shape == (128, c + 32 * (j - 1), 1, 1)
            assert sd[p + 'norm2.weight'].shape == (128,) and sd[p + 'conv2.weight'].shape == (32, 128, 3, 3)
        assert ('features.denseblock%d.denselayer%d.conv1.weight' % (i, n + 1)) not in sd
        c += 32 * n
        if i < 4:
            assert sd['features.transition%d.conv.weight' % i].shape == (c // 2, c, 1, 1)
            c //= 2
    assert sd['features.norm5.weight'].shape == (c,) and sd['classifier.weight'].shape == (1000, c)
    assert sd['features.conv0.weight'].shape == (64, 3, 7, 7)


def test_num_classes_kwarg_and_types_that_keep_raising():
    from robustart_amd.model import get_model
    assert get_model({'type': 'densenet121', 'kwargs': {'num_classes': 10, 'bn': {'use_sync_bn': False}}}).classifier.out_features == 10
    for t in ('mixer_l16_224', 'resnet18', 'resnext50_32x8d', 'convnext_large_cvst', 'vit_small_cvst', 'densenet161'):
        with pytest.raises(NotImplementedError, match='outside the hot-path scope') as e:
            get_model({'type': t})
        assert 'MLP-Mixer-B/16' in str(e.value)


def test_forward_of_a_tiny_module_matches_a_functional_restatement():
    """the module's forward against conv / batch-norm / concat / pool calls written out from the state dict, fp64"""
    import torch.nn.functional as F
    from robustart_amd.model.densenet_torch import DenseNet, randomize_bn_stats
    torch.manual_seed(0)
    cfg = (3, 2, 2, 1)
    m = randomize_bn_stats(DenseNet(cfg, num_classes=10)).eval().double()
    sd = m.state_dict()
    x = torch.randn(2, 3, 64, 64, dtype=torch.float64)

    def bn(y, p):
        return F.batch_norm(y, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'], False, 0.0, 1e-5)
    y = F.max_pool2d(F.relu(bn(F.conv2d(x, sd['features.conv0.weight'], stride=2, padding=3), 'features.norm0')), 3, 2, 1)
    for i, n in enumerate(cfg, 1):
        for j in range(1, n + 1):
            p = 'features.denseblock%d.denselayer%d.' % (i, j)
            a = F.conv2d(F.relu(bn(y, p + 'norm1')), sd[p + 'conv1.weight'])
            y = torch.cat([y, F.conv2d(F.relu(bn(a, p + 'norm2')), sd[p + 'conv2.weight'], padding=1)], 1)
        if i < 4:
            p = 'features.transition%d.' % i
            y = F.avg_pool2d(F.conv2d(F.relu(bn(y, p + 'norm')), sd[p + 'conv.weight']), 2, 2)
    want = F.linear(F.relu(bn(y, 'features.norm5')).mean((2, 3)), sd['classifier.weight'], sd['classifier.bias'])
    with torch.no_grad():
        got = m(x)
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


def test_new_symbols_are_declared_exported_and_bound():
    from robustart_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'robustart_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(rart_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.rart_version() == _lib.ABI_VERSION


def test_argument_checks_of_the_densenet_entries_without_gpu():
    """every check happens before a launch, so bad arguments return RART_ERR_INVALID (1) on a GPU-less box"""
    from robustart_amd import _lib
    lib = _lib.load()
    p, odd, n = _lib.c_void_p(4096), _lib.c_void_p(4104), None        # never dereferenced: the checks reject the call first

    def err(st, what):
        assert st == 1, what
        assert what.encode() in lib.rart_last_error_string(), lib.rart_last_error_string()
    # forward: (x, ld_x, s, t, y, sign, rows, c, stream) / pair: (x_hi, x_lo, ld_x, s, t, y_hi, y_lo, sign, rows, c, stream)
    err(lib.rart_dn_preact_bf16(n, 64, p, p, p, p, 10, 64, n), 'null tensor')
    err(lib.rart_dn_preact_bf16(p, 64, n, p, p, p, 10, 64, n), 'null tensor')
    err(lib.rart_dn_preact_pair(p, n, 64, p, p, p, p, p, 10, 64, n), 'null tensor')           # x_hi without x_lo
    err(lib.rart_dn_preact_pair(p, p, 64, p, p, p, n, p, 10, 64, n), 'null tensor')           # y_hi without y_lo
    err(lib.rart_dn_preact_bf16(p, 64, p, p, p, p, 0, 64, n), 'row count')
    err(lib.rart_dn_preact_bf16(p, 64, p, p, p, p, 1 << 31, 64, n), 'row count')
    err(lib.rart_dn_preact_bf16(p, 48, p, p, p, p, 10, 48, n), 'multiple of 32')
    err(lib.rart_dn_preact_bf16(p, 32, p, p, p, p, 10, 64, n), 'row stride')                  # ld < C
    err(lib.rart_dn_preact_bf16(p, 68, p, p, p, p, 10, 64, n), 'row stride')                  # ld % 8
    err(lib.rart_dn_preact_bf16(odd, 64, p, p, p, p, 10, 64, n), 'aligned')
    err(lib.rart_dn_preact_bf16(p, 64, p, p, p, _lib.c_void_p(4098), 10, 64, n), 'aligned')   # sign tensor: 4 bytes
    err(lib.rart_dn_preact_pair(p, p, 64, p, odd, p, p, p, 10, 64, n), 'aligned')
    # backward: (d, bits, s, g, ld_g, accumulate, rows, c, stream)
    err(lib.rart_dn_preact_bwd_bf16(p, n, p, p, 64, 0, 10, 64, n), 'null tensor')
    err(lib.rart_dn_preact_bwd_pair(p, p, p, n, p, n, 64, 0, 10, 64, n), 'null tensor')       # g_hi without g_lo
    err(lib.rart_dn_preact_bwd_bf16(p, p, n, p, 32, 0, 10, 64, n), 'ld_g')
    err(lib.rart_dn_preact_bwd_bf16(p, p, n, p, 64, 2, 10, 64, n), 'accumulate')
    err(lib.rart_dn_preact_bwd_bf16(p, p, n, p, 64, 1, 10, 40, n), 'multiple of 32')
    err(lib.rart_dn_preact_bwd_bf16(p, p, n, p, 64, 1, -1, 64, n), 'row count')
    err(lib.rart_dn_preact_bwd_bf16(p, p, n, odd, 64, 1, 10, 64, n), 'aligned')
    # the transition's pair: (x, ld_x, s, t, y, sign, n, h, w, c, stream) / (d, bits, s, g, ld_g, accumulate, n, h, w, c, stream)
    err(lib.rart_dn_preact_pool2_bf16(p, 64, p, p, p, p, 2, 7, 8, 64, n), 'even')
    err(lib.rart_dn_preact_pool2_bf16(p, 64, p, p, p, p, 0, 8, 8, 64, n), 'even')
    err(lib.rart_dn_preact_pool2_bf16(p, 64, p, p, n, p, 2, 8, 8, 64, n), 'null tensor')
    err(lib.rart_dn_preact_pool2_pair(p, p, 64, p, p, p, p, p, 2, 8, 8, 96, n), 'row stride')
    err(lib.rart_dn_preact_pool2_bf16(p, 64, p, p, p, p, 1 << 15, 1 << 8, 1 << 8, 64, n), 'row count')
    err(lib.rart_dn_preact_pool2_bwd_bf16(p, p, n, p, 64, 0, 2, 8, 9, 64, n), 'even')
    err(lib.rart_dn_preact_pool2_bwd_pair(p, p, p, n, p, p, 64, 3, 2, 8, 8, 64, n), 'accumulate')
    err(lib.rart_dn_preact_pool2_bwd_bf16(p, p, n, p, 56, 0, 2, 8, 8, 64, n), 'ld_g')
    # the slice copy: (src, ld_src, dst, ld_dst, rows, c, stream)
    err(lib.rart_dn_copy_bf16(p, 64, n, 64, 10, 64, n), 'null tensor')
    err(lib.rart_dn_copy_bf16(p, 64, p, 32, 10, 64, n), 'ld_dst')
    err(lib.rart_dn_copy_pair(p, p, 60, p, p, 64, 10, 64, n), 'row stride')
    err(lib.rart_dn_copy_pair(p, p, 64, p, odd, 64, 10, 64, n), 'aligned')


def test_make_engine_knows_densenet():
    """the dispatch names the DenseNet engine (building it needs a GPU: the error is the GPU check, not 'no HIP engine')"""
    from robustart_amd.model.densenet_engine import DenseNetEngine
    from robustart_amd.model.densenet_torch import DenseNet
    from robustart_amd.model.engine import ResNet50Engine, make_engine
    assert issubclass(DenseNetEngine, ResNet50Engine)          # it reuses the stem, the head and the GEMM launchers
    m = DenseNet((2, 2, 2, 2), num_classes=10).eval()
    if torch.cuda.is_available():
        assert isinstance(make_engine(m, 'cuda'), DenseNetEngine)
        return
    with pytest.raises(RuntimeError, match='no GPU visible'):
        make_engine(m, 'cuda')


@pytest.mark.parametrize('kw,what', [(dict(growth_rate=24), 'growth rate'), (dict(num_init_features=96), '64 channels'),
                                     (dict(growth_rate=32, bn_size=3, num_init_features=64, block_config=(2, 4)), None),
                                     (dict(block_config=(1, 2)), 'transition1'), (dict(bn_size=1, growth_rate=48), 'growth rate')])
def test_the_engine_refuses_widths_outside_its_scope_before_the_gpu(kw, what, monkeypatch):
    """a growth rate of 24, a 96-channel stem, a transition to 48 channels: NotImplementedError from the constructor, raised before
    the GPU check (and before any allocation); a module whose widths are all multiples of 32 passes on to that check"""
    from robustart_amd import _lib
    from robustart_amd.model.densenet_engine import DenseNetEngine
    from robustart_amd.model.densenet_torch import DenseNet

    def no_gpu():
        raise RuntimeError('reached the GPU check')
    monkeypatch.setattr(_lib, 'require_gpu', no_gpu)
    m = DenseNet(**dict(dict(block_config=(2, 2), num_classes=10), **kw)).eval()
    if what is None:
        with pytest.raises(RuntimeError, match='reached the GPU check'):
            DenseNetEngine(m, 'cuda')
        return
    with pytest.raises(NotImplementedError, match=what):
        DenseNetEngine(m, 'cuda')
    with pytest.raises(NotImplementedError, match=what):
        DenseNetEngine(m, 'cuda', precision='fp32x')


@pytest.mark.parametrize('t', sorted(PARAMS))
def test_training_a_densenet_is_refused_before_the_device(t, monkeypatch):
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
