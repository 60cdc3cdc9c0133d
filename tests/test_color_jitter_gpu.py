"""ColorJitter on the GPU: rart_color_jitter_u8 against Pillow (tests/_jitter_pil.py), byte for byte -- there is no tolerance in this
feature -- per operation on exhaustive inputs, composed in every order, in batches with different records, in place, between guard bytes
and with a dirty workspace; then FileImageNet built from the list-form transforms against Pillow's crop / resize / flip / jitter."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _jitter_pil import hue_shift, jitter_pil_plan      # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0xA5
BLEND_FACTORS = (0, 0.3, 0.8, 0.8001, 1, 1.2, 1.37, 0.123456789, 1.999)
ALL = dict(b=1.13, c=0.87, s=1.19, shift=240)


def _plan(order, b=None, c=None, s=None, shift=None):
    """(order, b, c, s, hue factor) of jitter.pack_jitter from a shift given as the uint8"""
    hf = None                                              # a factor inside the interval that truncates to the shift
    if shift is not None:
        hf = (shift + 0.5) / 255.0 if shift < 128 else (shift - 256 - 0.5) / 255.0
        assert -0.5 <= hf <= 0.5 and hue_shift(hf) == shift
    return (tuple(order) + tuple(o for o in range(4) if o not in order), b, c, s, hf)


def _launch(src, plans, pad=64, in_place=False, lsum=None):
    """the entry itself on a uint8 [n, h, w, 3] numpy batch; dst lies inside a larger buffer of guard bytes (pad on either side), which
    must survive; in_place: src is copied there first and the call gets dst == src"""
    from robustart_amd import _lib as L
    from robustart_amd.train.jitter import pack_jitter
    n, h, w, _ = src.shape
    nbytes = src.size
    buf = torch.full((nbytes + 2 * pad,), GUARD, dtype=torch.uint8, device='cuda')
    dst = buf[pad:pad + nbytes]
    s = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    if in_place:
        dst.copy_(s.view(-1))
        s = dst
    recs = torch.from_numpy(pack_jitter(plans)).cuda()
    if lsum is None:
        lsum = torch.empty(n, dtype=torch.int32, device='cuda')
    L.check(L.load().rart_color_jitter_u8(s.data_ptr(), dst.data_ptr(), n, h, w, recs.data_ptr(), lsum.data_ptr(), L.stream_ptr()))
    assert bool((buf[:pad] == GUARD).all()) and bool((buf[pad + nbytes:] == GUARD).all()), 'a store left dst'
    return dst.view(n, h, w, 3).cpu().numpy()


def _want(src, plans):
    return np.stack([a.copy() if p is None else jitter_pil_plan(a, p) for a, p in zip(src, plans)])


def _check(src, plans, **kw):
    got, want = _launch(src, plans, **kw), _want(src, plans)
    bad = int((got != want).any(-1).sum())
    assert bad == 0, '%d of %d pixels differ from Pillow; first at %s' % (bad, want[..., 0].size, np.argwhere((got != want).any(-1))[0])
    return got


_CACHE = {}


def _random(n, h, w):
    key = (n, h, w)
    if key not in _CACHE:
        _CACHE[key] = np.random.RandomState(n * 100003 + h * 1009 + w).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    return _CACHE[key]


def _cube():
    """all 2^24 RGB triples as one 4096 x 4096 image"""
    if 'cube' not in _CACHE:
        idx = np.arange(1 << 24, dtype=np.uint32)
        _CACHE['cube'] = np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], -1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    return _CACHE['cube']


# ---- one operation at a time ----------------------------------------------------------------------------------------------------------------
def test_brightness_on_every_byte_value_for_the_nine_blend_factors():
    """fp32 with the product and the sum rounded separately: a fused multiply-add or double arithmetic differs on some of these"""
    v = np.arange(256, dtype=np.uint8)
    img = np.stack([v, v[::-1], np.roll(v, 77)], -1).reshape(1, 16, 16, 3)
    for f in BLEND_FACTORS:
        _check(img, [_plan([0], b=float(f))])


@pytest.mark.parametrize('f', [0.8, 1.2])
def test_saturation_on_the_full_rgb_cube(f):
    _check(_cube(), [_plan([2], s=f)])


@pytest.mark.parametrize('shift', [0, 26, 231])
def test_hue_on_the_full_rgb_cube(shift):
    got = _check(_cube(), [_plan([3], shift=shift)])
    if shift == 0:
        same = float((got == _cube()).all(-1).mean())
        assert same < 0.5, 'the HSV round trip at shift 0 is not the identity (%.3f of the triples survive)' % same


def test_contrast_constant_random_half_and_odd_images():
    const = np.full((1, 8, 12, 3), 93, np.uint8)
    const[..., 1] = 17
    half = np.full((1, 4, 6, 3), 100, np.uint8)             # L mean exactly 100.5: m = 101
    half[:, :2] = 101
    for img in (const, _random(1, 16, 24), half, _random(1, 33, 17), _random(1, 7, 5), _random(1, 129, 67)):
        for f in (0.5, 0.8, 1.2, 1.999):
            _check(img, [_plan([1], c=f)])
    # the rounding decides bytes: with m = 100 the pixels of 101 would come out as 100 at f = 0.5
    got = _launch(half, [_plan([1], c=0.5)])
    assert got[0, 0, 0].tolist() == [101, 101, 101] and got[0, 3, 0].tolist() == [100, 100, 100]


# ---- composition ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(1, 1), (7, 5), (33, 17), (224, 224)])
def test_all_24_orders_with_all_four_operations(hw):
    orders = list(itertools.permutations(range(4)))
    src = _random(24, *hw)
    _check(src, [_plan(o, **ALL) for o in orders])


def test_batches_of_three_with_different_records():
    src = _random(3, 33, 17)
    for pos in range(4):                                    # contrast in every position, behind operations that change the mean
        order = [0, 2, 3]
        order.insert(pos, 1)
        plans = [_plan(order, **ALL),
                 _plan([2, 1, 0, 3], c=1.17, s=0.81),       # two operations inactive: their slots are skips
                 None]                                      # none: an exact copy
        got = _check(src, plans)
        assert np.array_equal(got[2], src[2])
    # and a record that is all skips although it names an order
    got = _check(src, [_plan([3, 1, 0, 2]), _plan([1], c=0.9), _plan([0, 1, 2, 3])])
    assert np.array_equal(got[0], src[0]) and np.array_equal(got[2], src[2])


def test_in_place_equals_out_of_place():
    for hw in ((33, 17), (64, 48)):
        src = _random(3, *hw)
        plans = [_plan([3, 0, 1, 2], **ALL), _plan([1, 2], c=1.2, s=0.8), _plan([2, 3, 1, 0], **ALL)]
        assert np.array_equal(_launch(src, plans, in_place=True), _check(src, plans))


def test_guard_bytes_survive_on_every_path():
    """_launch asserts the guards; here dst also starts at 1, 2 and 3 bytes past a dword (the byte path on full groups)"""
    plans = [_plan([0, 1, 2, 3], **ALL), _plan([3, 2, 1, 0], **ALL)]
    for hw in ((16, 16), (7, 5), (1, 1), (1, 3)):
        for pad in (64, 65, 66, 67):
            _check(_random(2, *hw), plans, pad=pad)
            _check(_random(2, *hw), plans, pad=pad, in_place=True)


def test_a_second_call_with_the_uncleared_workspace_gives_the_same_bytes():
    src = _random(3, 33, 17)
    plans = [_plan([0, 1, 2, 3], **ALL), _plan([1], c=1.3), _plan([3, 2, 1, 0], **ALL)]
    lsum = torch.full((3,), -1, dtype=torch.int32, device='cuda')             # dirty from the start
    first = _check(src, plans, lsum=lsum)
    r, g, b = (src[1, ..., c].astype(np.int64) for c in range(3))
    assert int(lsum[1]) == int(((19595 * r + 38470 * g + 7471 * b + 32768) >> 16).sum())     # the entry cleared the word itself
    assert np.array_equal(_launch(src, plans, lsum=lsum), first)


def test_apply_jitter_is_the_entry_and_reads_nothing_back():
    from robustart_amd.train.jitter import apply_jitter, draw_jitter, jitter_ranges
    ranges = jitter_ranges({'brightness': 0.2, 'contrast': 0.2, 'saturation': 0.2, 'hue': 0.1})
    src = _random(5, 33, 17)
    plans = [draw_jitter(ranges, 3, 1, i) for i in range(5)]
    want = _want(src, plans)
    dev = torch.from_numpy(src).cuda()
    out = torch.empty_like(dev)
    assert apply_jitter(dev, plans, out=out) is out and np.array_equal(out.cpu().numpy(), want) and np.array_equal(dev.cpu().numpy(), src)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        ret = apply_jitter(dev, plans)                      # in place
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert ret is dev and np.array_equal(dev.cpu().numpy(), want)
    with pytest.raises(ValueError):
        apply_jitter(dev, plans[:4])
    with pytest.raises(RuntimeError):
        apply_jitter(dev.cpu(), plans)


# ---- the solver's dataset ---------------------------------------------------------------------------------------------------------------------
def _png_set(tmp_path, n=4):
    from PIL import Image
    rs = np.random.RandomState(1)
    lines = []
    for i in range(n):
        Image.fromarray(rs.randint(0, 256, (70 + 9 * i, 96 - 5 * i, 3)).astype(np.uint8), 'RGB').save(str(tmp_path / ('im%d.png' % i)))
        lines.append('im%d.png %d' % (i, 10 + i))
    (tmp_path / 'meta.txt').write_text('\n'.join(lines) + '\n')
    return str(tmp_path), str(tmp_path / 'meta.txt')


def _pillow_standard(ds, indices, epoch, jitter, flip_on=True):
    """RandomResizedCrop + RandomHorizontalFlip [+ ColorJitter] by Pillow for the dataset's own draws"""
    from PIL import Image
    from robustart_amd.train.jitter import draw_jitter
    out = []
    for i in indices:
        arr, _ = ds.decode(i)
        y, x, h, w, flip = ds.box(i, arr.shape[:2], epoch)
        img = Image.fromarray(np.ascontiguousarray(arr[y:y + h, x:x + w]), 'RGB').resize((ds.size, ds.size), Image.BILINEAR)
        a = np.asarray(img)
        if flip and flip_on:
            a = a[:, ::-1]
        if jitter is not None:
            a = jitter_pil_plan(a, draw_jitter(jitter, ds.seed, epoch, i))
        out.append(np.ascontiguousarray(a))
    return np.stack(out)


def test_file_dataset_from_the_list_form_is_pillow_byte_for_byte(tmp_path):
    from robustart_amd.train import cls_solver as S
    root, meta = _png_set(tmp_path)
    norm = {'type': 'Normalize', 'kwargs': {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}}
    jit = {'type': 'ColorJitter', 'kwargs': {'brightness': 0.2, 'contrast': 0.2, 'saturation': 0.2, 'hue': 0.1}}
    lst = [{'type': 'RandomResizedCrop', 'kwargs': {'size': 64}}, {'type': 'RandomHorizontalFlip'}, jit, {'type': 'ToTensor'}, norm]
    dcfg = {'read_from': 'fs', 'input_size': 64, 'seed': 5, 'train': {'root_dir': root, 'meta_file': meta, 'transforms': lst}}
    ds = S.make_dataset(dcfg, 0, 64, 'train')
    idx = [2, 0, 3, 1]
    got, labs = ds.batch(idx, 'cuda', 1)
    assert labs.tolist() == [12, 10, 13, 11]
    assert np.array_equal(got.cpu().numpy(), _pillow_standard(ds, idx, 1, ds.jitter))
    again, _ = ds.batch(idx, 'cuda', 1)
    assert torch.equal(got, again)                                             # the same call twice: the same batch
    other, _ = ds.batch(idx, 'cuda', 2)
    assert not torch.equal(got, other)                                         # another epoch: another batch
    assert np.array_equal(other.cpu().numpy(), _pillow_standard(ds, idx, 2, ds.jitter))
    # the jitter is not ignored
    assert not np.array_equal(got.cpu().numpy(), _pillow_standard(ds, idx, 1, None))
    # a list without RandomHorizontalFlip never flips
    dcfg['train']['transforms'] = [lst[0], jit, lst[3], norm]
    nf = S.make_dataset(dcfg, 0, 64, 'train')
    assert any(nf.box(i, nf.decode(i)[0].shape[:2], e)[4] for i in idx for e in (0, 1, 2))      # some draws do ask for a flip
    for e in (0, 1, 2):
        assert np.array_equal(nf.batch(idx, 'cuda', e)[0].cpu().numpy(), _pillow_standard(nf, idx, e, nf.jitter, flip_on=False))
    # the mapping form returns what it returned before: crop, resize and flip, no jitter
    dcfg['train']['transforms'] = {'type': 'STANDARD'}
    mp = S.make_dataset(dcfg, 0, 64, 'train')
    for e in (0, 1):
        assert np.array_equal(mp.batch(idx, 'cuda', e)[0].cpu().numpy(), _pillow_standard(mp, idx, e, None))
    # the test list: Resize([72, 72]) + CenterCrop(64)
    from PIL import Image
    dcfg['test'] = {'root_dir': root, 'meta_file': meta,
                    'transforms': [{'type': 'Resize', 'kwargs': {'size': [72, 72]}}, {'type': 'CenterCrop', 'kwargs': {'size': [64, 64]}},
                                   {'type': 'ToTensor'}, norm]}
    te = S.make_dataset(dcfg, 0, 64, 'test')
    want = np.stack([np.asarray(Image.fromarray(te.decode(i)[0], 'RGB').resize((72, 72), Image.BILINEAR))[4:68, 4:68] for i in idx])
    assert np.array_equal(te.batch(idx, 'cuda')[0].cpu().numpy(), want)
