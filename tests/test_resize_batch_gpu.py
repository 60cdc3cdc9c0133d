"""The batched variable-size resize on the GPU: pil_resize_batch / rart_resize_batch_u8 and FileImageNet.batch on top of it against
Pillow alone (tests/_resize_batch_ref.py), bit for bit."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import _jpeg_decode_ref as J
import _resize_batch_ref as R

pytestmark = pytest.mark.gpu

FILTERS = range(6)


@pytest.fixture(scope='module')
def dev_sources():
    return [torch.from_numpy(np.array(x)).cuda() for x in R.sources()]


def _bad(got, want):
    got = got.cpu().numpy()
    return [k for k in range(len(want)) if got[k].shape != want[k].shape or not np.array_equal(got[k], want[k])]


@pytest.mark.parametrize('target,crop', [((36, 36), (2, 2, 32, 32)), ((29, 41), (3, 5, 20, 30))])
def test_mixed_sizes_every_filter_one_call(dev_sources, target, crop):
    from robustart_amd.noise import imagenet_s as S
    for f in FILTERS:
        before = S.resize_batch_launches
        got = S.pil_resize_batch(dev_sources, target, f, crop=crop)
        assert S.resize_batch_launches - before == 1
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (8, crop[2], crop[3], 3)
        assert not _bad(got, R.expected(target, f, crop)), ('filter %d' % f, _bad(got, R.expected(target, f, crop)))
    whole = S.pil_resize_batch(dev_sources, target, 1)                    # crop=None keeps the whole resized image
    assert not _bad(whole, R.expected(target, 1, None))


# per image: the full image, a 1 x 1 box, a box ending at the last row and column, boxes two columns wide (one more than 100 times
# as tall as wide, where Pillow runs the vertical pass first, and one that is not), an interior box
BOXES = ((0, 0, 1, 1), (1, 2, 1, 1), (7, 900, 30, 100), (100, 50, 800, 2), (0, 0, 75, 100), (30, 31, 6, 5), (5, 7, 25, 22), (10, 3, 150, 2))
FLIPS = (0, 1, 0, 1, 0, 1, 0, 1)


def test_boxes_and_flips(dev_sources):
    from robustart_amd.noise import imagenet_s as S
    for f in FILTERS:
        got = S.pil_resize_batch(dev_sources, (36, 36), f, crop=(2, 2, 32, 32), boxes=BOXES, flips=FLIPS)
        want = R.expected((36, 36), f, (2, 2, 32, 32), BOXES, FLIPS)
        assert not _bad(got, want), ('filter %d' % f, _bad(got, want))
    # the flip alone: the mirrored output of the unflipped call
    plain = S.pil_resize_batch(dev_sources, (36, 36), 2, boxes=BOXES)
    flipped = S.pil_resize_batch(dev_sources, (36, 36), 2, boxes=BOXES, flips=[1] * 8)
    assert torch.equal(flipped, plain.flip(2))


def test_the_box_is_a_hard_boundary(dev_sources):
    """make_image(3, 33, 47), the box x 5..30, y 7..29, LANCZOS to 32 x 32: Image.resize(box=...) reads outside the box for its filter
    support, crop-then-resize does not; the two must differ visibly for this input to tell them apart, and the kernel is the latter"""
    from robustart_amd.noise import imagenet_s as S
    from _inputs import make_image
    x = make_image(3, 33, 47)
    box = (7, 5, 22, 25)                                                   # (y, x, h, w)
    hard = R.pillow(x, (32, 32), 5, box=box)
    soft = R.pillow_box_argument(x, (32, 32), 5, box)
    differ = float((hard != soft).mean())
    print('crop-then-resize vs Image.resize(box=): %.1f %% of the bytes differ' % (100 * differ))
    assert differ >= 0.10
    got = S.pil_resize_batch([torch.from_numpy(x).cuda()], (32, 32), 5, boxes=[box])
    assert np.array_equal(got[0].cpu().numpy(), hard)


def test_position_and_company_do_not_matter(dev_sources):
    from robustart_amd.noise import imagenet_s as S
    k = 4                                                                   # 75 x 100
    others = [s for j, s in enumerate(dev_sources) if j != k]
    img = dev_sources[k]
    packed = torch.cat([s.reshape(-1) for s in dev_sources])               # the sources as views of one packed buffer
    views, off = [], 0
    for s in dev_sources:
        views.append(packed[off:off + s.numel()].view(s.shape))
        off += s.numel()
    for f in FILTERS:
        crop = (2, 2, 32, 32)
        first = S.pil_resize_batch([img] + others, (36, 36), f, crop=crop)[0]
        middle = S.pil_resize_batch(others[:3] + [img] + others[3:], (36, 36), f, crop=crop)[3]
        last = S.pil_resize_batch(others + [img], (36, 36), f, crop=crop)[7]
        alone = S.pil_resize_batch([img], (36, 36), f, crop=crop)[0]
        single = S.pil_resize(img[None], (36, 36), f, crop=crop)[0]
        assert torch.equal(first, middle) and torch.equal(first, last) and torch.equal(first, alone) and torch.equal(first, single), f
        a = S.pil_resize_batch(views, (36, 36), f, crop=crop, boxes=BOXES, flips=FLIPS)
        b = S.pil_resize_batch(dev_sources, (36, 36), f, crop=crop, boxes=BOXES, flips=FLIPS)
        assert torch.equal(a, b), f
    out = torch.full((8, 32, 32, 3), 9, dtype=torch.uint8, device='cuda')
    assert S.pil_resize_batch(dev_sources, (36, 36), 1, crop=(2, 2, 32, 32), out=out) is out          # fills the caller's batch in place
    assert not _bad(out, R.expected((36, 36), 1, (2, 2, 32, 32)))


def test_refusals_before_any_launch(dev_sources):
    from robustart_amd import _lib
    lib = _lib.load()
    imgs = [dev_sources[6], dev_sources[4]]                                # 33 x 47, 75 x 100
    target, crop = (36, 36), (2, 2, 32, 32)

    def descs(boxes=(None, None)):
        d = (_lib.ResizeDesc * 2)()
        for k, im in enumerate(imgs):
            d[k].src, d[k].h, d[k].w = im.data_ptr(), im.shape[0], im.shape[1]
            d[k].box_y, d[k].box_x, d[k].box_h, d[k].box_w = boxes[k] or (0, 0, im.shape[0], im.shape[1])
        return d

    def plan(d, n=2, f=5, crop=crop, buf=None):
        sizes = _lib.ResizePlan()
        st = lib.rart_resize_batch_plan(ctypes.addressof(d), n, f, target[0], target[1], *crop, None if buf is None else buf.ctypes.data,
                                        0 if buf is None else buf.size, ctypes.byref(sizes))
        return st, sizes

    def err():
        return lib.rart_last_error_string()

    # the plan entry refuses the caller's mistakes
    assert plan(descs(), n=0)[0] == 1 and b'count' in err()
    assert plan(descs(), f=6)[0] == 1 and b'filter' in err()
    assert plan(descs(((0, 0, 34, 47), None)))[0] == 1 and b'box' in err()                 # one row past the image
    assert plan(descs((None, (0, 1, 75, 100))))[0] == 1 and b'box' in err()                # one column past the image
    assert plan(descs(), crop=(2, 5, 32, 32))[0] == 1 and b'crop window' in err()          # one column past the target
    assert plan(descs(), crop=(5, 2, 32, 32))[0] == 1 and b'crop window' in err()
    st, sizes = plan(descs())
    assert st == 0
    short = np.zeros(sizes.total_bytes - 1, np.uint8)
    assert plan(descs(), buf=short[:short.size // 16 * 16])[0] == 3 and b'plan buffer' in err()
    host = np.zeros(sizes.total_bytes, np.uint8)
    assert plan(descs(), buf=host)[0] == 0
    dplan = torch.from_numpy(host).cuda()
    need = int(sizes.workspace_bytes)
    assert need > 0
    ws = torch.full((need,), 7, dtype=torch.uint8, device='cuda')
    out = torch.full((2, 32, 32, 3), 7, dtype=torch.uint8, device='cuda')

    def call(h=host, ws_bytes=need, out_bytes=out.numel()):
        return lib.rart_resize_batch_u8(_lib.ptr(dplan), h.ctypes.data, h.size, _lib.ptr(ws), ws_bytes, _lib.ptr(out), out_bytes,
                                        _lib.stream_ptr())

    def edited(offset, ctype, value):
        h = host.copy()
        ctype.from_buffer(h, offset).value = value
        return h

    P, D = _lib.ResizePlan, _lib.ResizeDesc
    # the device entry refuses a host copy that says any of this, and a workspace / output one byte short
    assert call(edited(P.n.offset, ctypes.c_int32, 0)) == 1 and b'count' in err()
    assert call(edited(P.filter.offset, ctypes.c_int32, 6)) == 1 and b'filter' in err()
    assert call(edited(sizes.desc_off + D.box_h.offset, ctypes.c_int32, 34)) == 1 and b'box' in err()
    assert call(edited(sizes.desc_off + ctypes.sizeof(D) + D.box_x.offset, ctypes.c_int32, 1)) == 1 and b'box' in err()
    assert call(edited(P.crop_x.offset, ctypes.c_int32, 5)) == 1 and b'crop window' in err()
    assert call(ws_bytes=need - 1) == 3 and b'workspace' in err()
    assert call(out_bytes=out.numel() - 1) == 1 and b'out of' in err()
    assert call(edited(sizes.desc_off + D.tab_v.offset, ctypes.c_int32, int(sizes.table_count))) == 1 and b'table offset' in err()
    assert call(edited(sizes.desc_off + ctypes.sizeof(D) + D.tab_h.offset, ctypes.c_int32, int(sizes.table_count) - 8)) == 1 and b'table offset' in err()
    assert call(edited(sizes.prefix_off + 8, ctypes.c_int64, 1 << 40)) == 1 and b'prefix' in err()
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and bool((out == 7).all())               # nothing was launched
    assert call() == 0
    want = [R.pillow(np.array(R.sources()[k]), target, 5, crop) for k in (6, 4)]
    assert not _bad(out, want)


SPECS = [('444', 37, 53), ('422', 65, 47), ('420', 48, 40), ('gray', 31, 33), ('420_rst', 100, 75), ('420_q95', 17, 23),
         ('420_opt_q30', 120, 90), ('422', 24, 35), ('420', 375, 500), ('444', 64, 64), ('progressive', 50, 70), ('png', 40, 60)]


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    """three class folders, 12 files of 17 x 23 up to 375 x 500: 10 baseline JPEGs (all samplings, one grayscale, one with restart
    markers), one progressive JPEG and one PNG"""
    root = tmp_path_factory.mktemp('resize_folder')
    for k, (kind, h, w) in enumerate(SPECS):
        d = root / ('class%d' % (k % 3))
        d.mkdir(exist_ok=True)
        arr = J.source_array(h, w, 'smooth' if k % 2 else 'noise', seed=4)
        if kind == 'progressive':
            Image.fromarray(arr).save(str(d / ('img%02d.jpg' % k)), 'JPEG', progressive=True)
        elif kind == 'png':
            Image.fromarray(arr).save(str(d / ('img%02d.png' % k)), 'PNG')
        else:
            (d / ('img%02d.jpg' % k)).write_bytes(J.encode(arr, kind))
    return str(root)


@pytest.mark.parametrize('reader', ['pil', 'hip'])
@pytest.mark.parametrize('transform', ['ONECROP', 'STANDARD'])
def test_public_path_against_pillow_alone(folder, transform, reader, monkeypatch):
    """FileImageNet.batch = the transform restated with Pillow: decode, then crop(box) / resize / mirror, or resize to [73, 73] and
    centre crop; one rart_resize_batch_u8 call per batch() and no per-image pil_resize call"""
    import os
    from robustart_amd.noise import imagenet_s as S
    from robustart_amd.train.cls_solver import FileImageNet
    singles = []
    real = S.pil_resize
    monkeypatch.setattr(S, 'pil_resize', lambda *a, **k: (singles.append(1), real(*a, **k))[1])
    ds = FileImageNet.from_folder(folder, 64, 73, transform, reader, seed=5)
    assert len(ds) == 12
    flips = 0
    for epoch in (0, 1):
        before = S.resize_batch_launches
        got, labels = ds.batch(range(12), 'cuda', epoch)
        assert S.resize_batch_launches - before == 1 and not singles
        assert tuple(got.shape) == (12, 64, 64, 3) and labels.tolist() == [lab for _, lab in ds.items]
        want = []
        for i, (name, _) in enumerate(ds.items):
            with Image.open(os.path.join(folder, name)) as im:
                arr = np.array(im.convert('RGB'))
            if transform == 'ONECROP':
                want.append(R.pillow(arr, (73, 73), 1, crop=(4, 4, 64, 64)))              # round((73 - 64) / 2) = 4
            else:
                y, x, h, w, flip = ds.box(i, arr.shape[:2], epoch)
                flips += int(flip)
                want.append(R.pillow(arr, (64, 64), 1, box=(y, x, h, w), flip=flip))
        assert not _bad(got, want), (transform, reader, epoch, _bad(got, want))
    assert transform == 'ONECROP' or 0 < flips < 24                        # the draws do ask for some flips
