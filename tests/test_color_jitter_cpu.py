"""List-form `data.<split>.transforms` and ColorJitter (robustart_amd/train/jitter.py, cls_solver.read_transforms) without a GPU: the
library entry is declared, exported and bound and checks its arguments before any launch; the ranges are validated as torchvision
validates them; the draws are a pure function of (seed, epoch, index); the packed records have the header's layout; and the transforms
reader maps the reference's list-form config to the arguments FileImageNet takes, refusing what this build does not compute."""
import ctypes
import copy
import os
import re

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'transforms_list_ref.yaml')     # the data: block of imagenet_s_loop/config_convnext_base.yaml


def test_new_symbol_is_declared_exported_and_bound():
    from robustart_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'robustart_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(rart_[a-z0-9_]+)\s*\(', src))
    lib = _lib.load()
    s = 'rart_color_jitter_u8'
    assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s)
    assert lib.rart_version() == 110 == _lib.ABI_VERSION
    assert 'rart_jitter_rec' in src and ctypes.sizeof(_lib.JitterRec) == 20
    assert (_lib.JitterRec.op.offset, _lib.JitterRec.factor.offset, _lib.JitterRec.hue_shift.offset) == (0, 4, 16)


def test_argument_checks_without_gpu():
    """every check happens before the workspace is cleared or a kernel launched; the pointers are never dereferenced"""
    from robustart_amd import _lib
    lib = _lib.load()
    p, q, r, w = 4096, 1 << 40, 1 << 41, 1 << 42
    cj = lambda *a: lib.rart_color_jitter_u8(*a, None)           # noqa: E731
    err = lib.rart_last_error_string
    for src, dst, par, ws in ((None, q, r, w), (p, None, r, w), (p, q, None, w), (p, q, r, None)):
        assert cj(src, dst, 2, 8, 12, par, ws) == 1 and b'null' in err()
    for n, h, wd in ((0, 8, 12), (-1, 8, 12), (2, 0, 12), (2, 8, -4)):
        assert cj(p, q, n, h, wd, r, w) == 1 and b'positive' in err()
    # the 32-bit luminance sum: 2^24 pixels of L = 255 are the most that fit
    assert cj(p, q, 1, 4096, 4097, r, w) == 1 and b'too large' in err()
    assert cj(p, q, 1, 1 << 12, (1 << 12) + 1, r, w) == 1
    assert cj(p, q, 1, 1 << 20, 1 << 20, r, w) == 1 and b'too large' in err()            # h * w overflows 32 bits
    # 2^32 bytes or more: 29000 x 224 x 224 x 3 = 4.4e9
    assert cj(p, q, 29000, 224, 224, r, w) == 1 and b'too many' in err()
    # partial overlap: 2 * 8 * 12 * 3 = 576 bytes; dst starting or ending inside src
    for d in (q + 1, q + 575, q - 1, q - 575):
        assert cj(q, d, 2, 8, 12, r, w) == 1 and b'overlap' in err(), d


# ---- ranges -------------------------------------------------------------------------------------------------------------------------------
def test_jitter_ranges_as_torchvision_validates_them():
    from robustart_amd.train.jitter import jitter_ranges
    got = jitter_ranges({'brightness': 0.2, 'contrast': 0.2, 'saturation': 0.2, 'hue': 0.1})
    assert got == ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))
    assert jitter_ranges({'brightness': 1.5}) == ((0.0, 2.5), None, None, None)                  # the lower end is clipped at 0
    assert jitter_ranges({'hue': 0.5}) == (None, None, None, (-0.5, 0.5))
    assert jitter_ranges({'brightness': 0, 'contrast': 0.0, 'saturation': 0, 'hue': 0}) is None    # 0 is inactive
    assert jitter_ranges({}) is None and jitter_ranges(None) is None
    assert jitter_ranges({'contrast': [0.5, 1.5], 'hue': (-0.2, 0.3)}) == (None, (0.5, 1.5), None, (-0.2, 0.3))
    assert jitter_ranges({'saturation': [1, 1], 'hue': [0, 0], 'brightness': [1.0, 1.25]}) == ((1.0, 1.25), None, None, None)
    assert jitter_ranges({'saturation': [2, 2]}) == (None, None, (2.0, 2.0), None)                # degenerate but not neutral: active
    bad = [('brightness', -0.1), ('contrast', [-0.1, 1.0]), ('saturation', [1.2, 0.8]), ('hue', 0.6), ('hue', [-0.6, 0.1]),
           ('hue', [0.2, 0.1]), ('hue', -0.1), ('brightness', 'a lot'), ('contrast', [1.0]), ('saturation', [0.5, 1.0, 1.5]),
           ('brightness', float('nan'))]
    for key, v in bad:
        with pytest.raises(ValueError, match=key):
            jitter_ranges({key: v})
    with pytest.raises(ValueError, match='gamma'):
        jitter_ranges({'gamma': 0.1})


# ---- draws --------------------------------------------------------------------------------------------------------------------------------
RANGES = ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))


def test_draw_jitter_is_a_pure_function_of_its_key():
    from robustart_amd.train.jitter import draw_jitter
    a = draw_jitter(RANGES, 3, 7, 11)
    np.random.seed(5)                                       # global generator state plays no part
    draw_jitter(RANGES, 3, 7, 12)                           # nor do earlier calls
    assert draw_jitter(RANGES, 3, 7, 11) == a
    for other in ((4, 7, 11), (3, 8, 11), (3, 7, 12)):      # another seed, epoch, index: another plan
        assert draw_jitter(RANGES, *other) != a
    order, b, c, s, h = a
    assert sorted(order) == [0, 1, 2, 3] and all(isinstance(v, float) for v in (b, c, s, h))


def test_draws_cover_all_orders_and_stay_in_range():
    from robustart_amd.train.jitter import draw_jitter, hue_shift
    orders = set()
    for i in range(2000):
        order, b, c, s, h = draw_jitter(RANGES, 0, i // 500, i)
        orders.add(order)
        assert 0.8 <= b <= 1.2 and 0.8 <= c <= 1.2 and 0.8 <= s <= 1.2 and -0.1 <= h <= 0.1
        assert hue_shift(h) in set(range(0, 26)) | set(range(231, 256))
    assert len(orders) == 24
    # inactive operations draw nothing and come back as None; the order is still a full permutation
    order, b, c, s, h = draw_jitter(((0.5, 1.5), None, None, (-0.5, 0.5)), 0, 0, 0)
    assert sorted(order) == [0, 1, 2, 3] and c is None and s is None and 0.5 <= b <= 1.5 and -0.5 <= h <= 0.5
    assert hue_shift(0.1) == 25 and hue_shift(-0.1) == 231 and hue_shift(0.0) == 0 and hue_shift(-0.001) == 0 and hue_shift(0.5) == 127


def test_pack_jitter_writes_the_header_layout_and_validates():
    from robustart_amd.train.jitter import SKIP, pack_jitter
    recs = pack_jitter([((2, 0, 3, 1), 1.1, None, 0.9, -0.1), None, ((3, 2, 1, 0), None, 0.5, None, None)])
    assert recs.dtype == np.uint8 and recs.shape == (3, 20)
    assert recs[0, :4].tolist() == [2, 0, 3, SKIP]                                         # contrast is inactive: its slot is a skip
    assert recs[0, 4:16].view(np.float32).tolist() == [np.float32(1.1), 0.0, np.float32(0.9)]
    assert int(recs[0, 16:20].view(np.uint32)[0]) == 231
    assert recs[1, :4].tolist() == [SKIP] * 4
    assert recs[2, :4].tolist() == [SKIP, SKIP, 1, SKIP] and recs[2, 4:16].view(np.float32).tolist() == [0.0, 0.5, 0.0]
    for plan in (((0, 0, 1, 2), 1.0, 1.0, 1.0, 0.0), ((0, 1, 2, 4), 1.0, 1.0, 1.0, 0.0), ((0, 1, 2, 3), -0.5, 1.0, 1.0, 0.0),
                 ((0, 1, 2, 3), 1.0, float('nan'), 1.0, 0.0), ((0, 1, 2, 3), 1.0, 1.0, float('inf'), 0.0), ((0, 1, 2, 3), 1.0, 1.0, 1.0, 0.6)):
        with pytest.raises(ValueError):
            pack_jitter([plan])


def test_apply_jitter_has_no_cpu_fallback():
    from robustart_amd.train.jitter import apply_jitter
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        apply_jitter(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), [None])


# ---- the transforms reader ----------------------------------------------------------------------------------------------------------------
def _ref_data():
    return yaml.safe_load(open(FIXTURE))['data']


def test_reference_lists_map_to_standard_with_ranges_and_onecrop_256():
    from robustart_amd.train.cls_solver import read_transforms
    d = _ref_data()
    assert isinstance(d['train']['transforms'], list) and isinstance(d['test']['transforms'], list)
    assert read_transforms(d, 'train') == {'type': 'STANDARD', 'test_resize': 256, 'jitter': RANGES, 'flip': True}
    assert read_transforms(d, 'test') == {'type': 'ONECROP', 'test_resize': 256, 'jitter': None, 'flip': True}
    # Resize(r) and another r; the list's r wins over data.test_resize
    d['test']['transforms'][0]['kwargs']['size'] = 232
    d['test_resize'] = 300
    assert read_transforms(d, 'test')['test_resize'] == 232
    # a list without the flip never flips; without the jitter there are no ranges
    d['train']['transforms'] = [e for e in d['train']['transforms'] if e['type'] not in ('RandomHorizontalFlip', 'ColorJitter')]
    assert read_transforms(d, 'train') == {'type': 'STANDARD', 'test_resize': 300, 'jitter': None, 'flip': False}


def _png_set(tmp_path, n=3):
    from PIL import Image
    rs = np.random.RandomState(0)
    lines = []
    for i in range(n):
        Image.fromarray(rs.randint(0, 256, (40 + 3 * i, 52 - i, 3)).astype(np.uint8), 'RGB').save(str(tmp_path / ('im%d.png' % i)))
        lines.append('im%d.png %d' % (i, i))
    (tmp_path / 'meta.txt').write_text('\n'.join(lines) + '\n')
    return str(tmp_path), str(tmp_path / 'meta.txt')


def test_make_dataset_builds_from_the_reference_lists(tmp_path):
    """fails with AttributeError ('list' object has no attribute 'get') on a solver that reads the key as a mapping only"""
    from robustart_amd.train.cls_solver import FileImageNet, make_dataset
    root, meta = _png_set(tmp_path)
    d = _ref_data()
    for split in ('train', 'test'):
        d[split]['root_dir'], d[split]['meta_file'] = root, meta
    tr = make_dataset(d, 0, 224, 'train')
    assert isinstance(tr, FileImageNet) and len(tr) == 3
    assert (tr.transform, tr.jitter, tr.flip, tr.size) == ('STANDARD', RANGES, True, 224)
    te = make_dataset(d, 0, 224, 'test')
    assert isinstance(te, FileImageNet) and (te.transform, te.jitter, te.test_resize, te.size) == ('ONECROP', None, 256, 224)


def test_mapping_form_reads_as_before(tmp_path):
    from robustart_amd.train.cls_solver import make_dataset, read_transforms
    root, meta = _png_set(tmp_path)
    sec = {'root_dir': root, 'meta_file': meta}
    for split, given, want in (('test', None, 'ONECROP'), ('train', None, 'STANDARD'), ('test', {'type': 'STANDARD'}, 'STANDARD'),
                               ('train', {'type': 'ONECROP'}, 'ONECROP'), ('train', {}, 'STANDARD'), ('test', [], 'ONECROP')):
        d = {'read_from': 'fs', 'test_resize': 232, 'seed': 4, split: dict(sec)}
        if given is not None:
            d[split]['transforms'] = given
        assert read_transforms(d, split) == {'type': want, 'test_resize': 232, 'jitter': None, 'flip': True}
        ds = make_dataset(d, 0, 64, split)
        assert (ds.transform, ds.test_resize, ds.jitter, ds.flip, ds.seed, ds.size) == (want, 232, None, True, 4, 64)
    with pytest.raises(NotImplementedError, match='FIVECROP'):
        make_dataset({'read_from': 'fs', 'test': dict(sec, transforms={'type': 'FIVECROP'})}, 0, 64, 'test')


def test_refusals():
    from robustart_amd.train.cls_solver import read_transforms
    ref = _ref_data()

    def with_(split, fn):
        d = copy.deepcopy(ref)
        fn(d[split]['transforms'])
        return d

    # a non-square Resize
    d = with_('test', lambda t: t[0]['kwargs'].update(size=[256, 320]))
    with pytest.raises(NotImplementedError, match='non-square Resize'):
        read_transforms(d, 'test')
    # Normalize with another mean or std
    for key, v in (('mean', [0.5, 0.5, 0.5]), ('std', [0.25, 0.25, 0.25])):
        for split in ('train', 'test'):
            d = with_(split, lambda t: t[-1]['kwargs'].update({key: v}))
            with pytest.raises(NotImplementedError, match='ImageNet constants'):
                read_transforms(d, split)
    # any other entry type, named
    for split, entry in (('train', {'type': 'RandomErasing'}), ('test', {'type': 'FiveCrop', 'kwargs': {'size': 224}}),
                         ('train', {'type': 'AutoAugment'})):
        d = with_(split, lambda t: t.insert(1, entry))
        with pytest.raises(NotImplementedError, match=entry['type']):
            read_transforms(d, split)
    # sizes other than data.input_size
    d = with_('train', lambda t: t[0]['kwargs'].update(size=192))
    with pytest.raises(ValueError, match='RandomResizedCrop size'):
        read_transforms(d, 'train')
    d = with_('test', lambda t: t[1]['kwargs'].update(size=[192, 192]))
    with pytest.raises(ValueError, match='CenterCrop size'):
        read_transforms(d, 'test')
    d = copy.deepcopy(ref)
    d['input_size'] = 192
    with pytest.raises(ValueError, match='RandomResizedCrop size'):
        read_transforms(d, 'train')
    # entries out of place
    d = with_('train', lambda t: t.insert(1, t.pop(2)))                       # ColorJitter before RandomHorizontalFlip
    with pytest.raises(ValueError, match='out of place'):
        read_transforms(d, 'train')
    d = with_('test', lambda t: t.insert(2, {'type': 'ColorJitter', 'kwargs': {'hue': 0.1}}))
    with pytest.raises(ValueError, match='test list'):
        read_transforms(d, 'test')
    d = with_('train', lambda t: t.pop())                                     # no Normalize
    with pytest.raises(ValueError, match='ToTensor, Normalize'):
        read_transforms(d, 'train')
    # the jitter's own validation surfaces with the key's name
    d = with_('train', lambda t: t[2]['kwargs'].update(hue=0.7))
    with pytest.raises(ValueError, match='hue'):
        read_transforms(d, 'train')
    # neither a mapping nor a list
    d = copy.deepcopy(ref)
    d['train']['transforms'] = 'STANDARD'
    with pytest.raises(ValueError, match='mapping'):
        read_transforms(d, 'train')
