"""The batched variable-size OpenCV resize on the GPU: cv_resize_batch / rart_cv_resize_batch_u8 and image_transfer_batch on top of it
against oracle/resize_cv_np.py and the per-image cv_resize, bit for bit.  Sources are noise images, where the five operators differ
nearly everywhere."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

INTERPS = range(5)                                     # cv2.INTER_NEAREST, LINEAR, CUBIC, AREA, LANCZOS4
NAMES = ['opencv-nearest', 'opencv-bilinear', 'opencv-cubic', 'opencv-area', 'opencv-lanczos']
SIZES = [(72, 72), (108, 72), (75, 100), (33, 47), (20, 25), (36, 36), (75, 100), (72, 90), (900, 7), (1, 1), (30, 1), (144, 36),
         (37, 35), (72, 72)]
TARGET, CROP = (36, 36), (2, 2, 32, 32)


def _noise(k, h, w):
    return np.random.default_rng(1000 + k).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _oracle(arr, target, interp, crop=None, box=None, flip=False):
    from oracle import resize_cv_np as CV
    if box is not None:
        arr = arr[box[0]:box[0] + box[2], box[1]:box[1] + box[3]]
    r = CV.resize(np.ascontiguousarray(arr), (target[1], target[0]), interp)
    if crop is not None:
        r = r[crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]]
    return r[:, ::-1] if flip else r


@pytest.fixture(scope='module')
def sources():
    return [_noise(k, h, w) for k, (h, w) in enumerate(SIZES)]


@pytest.fixture(scope='module')
def dev_sources(sources):
    return [torch.from_numpy(a).cuda() for a in sources]


@pytest.fixture(scope='module')
def whole(sources):
    """whole[interp][k]: the oracle's 36 x 36 resize of source k, computed once"""
    return [[_oracle(a, TARGET, f) for a in sources] for f in INTERPS]


def _bad(got, want):
    got = got.cpu().numpy()
    return [k for k in range(len(want)) if got[k].shape != want[k].shape or not np.array_equal(got[k], want[k])]


def _cropped(rows, crop):
    return [r if crop is None else r[crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]] for r in rows]


def test_the_sources_tell_the_operators_apart(whole):
    """by the oracle alone: on every image but (36, 36) and (1, 1), any two operators differ in at least 25 % of the bytes, except
    LINEAR / AREA on (72, 72), which cv2 executes with the same code -- so a batch that mixed up its operators or paths cannot pass"""
    smallest = 1.0
    for k, hw in enumerate(SIZES):
        for a in INTERPS:
            for b in range(a + 1, 5):
                differ = float((whole[a][k] != whole[b][k]).mean())
                if hw in ((36, 36), (1, 1)) or (hw == (72, 72) and (a, b) == (1, 3)):
                    assert differ == 0.0, (hw, a, b)                      # equal by definition
                    continue
                smallest = min(smallest, differ)
                assert differ >= 0.25, (hw, a, b, differ)
    print('smallest share of differing bytes between two operators: %.1f %%' % (100 * smallest))


@pytest.mark.parametrize('crop', [CROP, None])
def test_mixed_batch_every_interpolation_one_call(dev_sources, whole, crop):
    from robustart_amd.noise import imagenet_s as S
    shape = (14,) + ((crop[2], crop[3]) if crop else TARGET) + (3,)
    for f in INTERPS:
        before = S.cv_resize_batch_launches
        got = S.cv_resize_batch(dev_sources, TARGET, f, crop=crop)
        assert S.cv_resize_batch_launches - before == 1
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == shape
        want = _cropped(whole[f], crop)
        assert not _bad(got, want), ('interpolation %d' % f, _bad(got, want))
        single = torch.stack([S.cv_resize(d[None], TARGET, f, crop=crop)[0] for d in dev_sources])
        assert torch.equal(got, single), ('interpolation %d' % f, _bad(got, list(single.cpu().numpy())))


# boxes strictly inside their images, so a clamp to the image instead of the box reads other pixels; three change their image's path
# under AREA: (75, 100) becomes integer-area with a row stride that is not the box width, (108, 72) float-area, (900, 7) stays two-pass
# with a box two columns wide; (1, 1) and (30, 1) have no interior
BOXES = [(1, 1, 70, 70), (3, 0, 100, 70), (1, 2, 72, 72), (2, 3, 30, 40), None, (1, 1, 34, 34), (5, 7, 60, 80), (1, 1, 70, 88),
         (100, 2, 800, 2), None, None, (1, 1, 142, 34), (1, 1, 35, 33), (2, 2, 37, 61)]
FLIPS = [k % 2 for k in range(14)]


def test_boxes_and_mirrors(sources, dev_sources):
    from robustart_amd.noise import imagenet_s as S
    for f in INTERPS:
        got = S.cv_resize_batch(dev_sources, TARGET, f, crop=CROP, boxes=BOXES, flips=FLIPS)
        want = [_oracle(a, TARGET, f, CROP, b, fl) for a, b, fl in zip(sources, BOXES, FLIPS)]
        assert not _bad(got, want), ('interpolation %d' % f, _bad(got, want))
    # the flip alone: the mirrored output of the unflipped call
    plain = S.cv_resize_batch(dev_sources, TARGET, 3, boxes=BOXES)
    flipped = S.cv_resize_batch(dev_sources, TARGET, 3, boxes=BOXES, flips=[1] * 14)
    assert torch.equal(flipped, plain.flip(2))


def test_packed_sources_at_unaligned_offsets(dev_sources):
    """every image a view into one uint8 buffer at consecutive byte offsets (3 h w each: most are not multiples of 4)"""
    from robustart_amd.noise import imagenet_s as S
    packed = torch.cat([s.reshape(-1) for s in dev_sources])
    views, off = [], 0
    for s in dev_sources:
        views.append(packed[off:off + s.numel()].view(s.shape))
        off += s.numel()
    assert sum(v.data_ptr() % 4 != 0 for v in views) >= 4
    for f in INTERPS:
        a = S.cv_resize_batch(views, TARGET, f, crop=CROP, boxes=BOXES, flips=FLIPS)
        b = S.cv_resize_batch(dev_sources, TARGET, f, crop=CROP, boxes=BOXES, flips=FLIPS)
        assert torch.equal(a, b), f


def test_one_image_and_thirty_three(dev_sources, whole):
    from robustart_amd.noise import imagenet_s as S
    order = [(7 * j + 3) % 14 for j in range(33)]                       # sizes repeat; more than one bisection level
    for f in INTERPS:
        for k in (2, 3, 9):                                               # under AREA: float-area, two-pass, two-pass on 1 x 1
            alone = S.cv_resize_batch([dev_sources[k]], TARGET, f, crop=CROP)
            assert not _bad(alone, _cropped([whole[f][k]], CROP)), (f, k)
        got = S.cv_resize_batch([dev_sources[k] for k in order], TARGET, f, crop=CROP)
        want = _cropped([whole[f][k] for k in order], CROP)
        assert not _bad(got, want), (f, _bad(got, want))


def test_out_argument_guard_bands_and_refusals(dev_sources, whole):
    from robustart_amd.noise import imagenet_s as S
    big = torch.full((16, 32, 32, 3), 0xA5, dtype=torch.uint8, device='cuda')
    for f in INTERPS:
        big.fill_(0xA5)
        out = big[1:15]
        assert S.cv_resize_batch(dev_sources, TARGET, f, crop=CROP, out=out) is out
        assert bool((big[0] == 0xA5).all()) and bool((big[15] == 0xA5).all()), f
        assert not _bad(out, _cropped(whole[f], CROP)), f
    before = S.cv_resize_batch_launches
    with pytest.raises(ValueError, match='out must be'):
        S.cv_resize_batch(dev_sources, TARGET, 1, crop=CROP, out=big[:14, :31])
    with pytest.raises(ValueError, match='out must be'):
        S.cv_resize_batch(dev_sources, TARGET, 1, crop=CROP, out=big[:13])
    with pytest.raises(ValueError, match='out must be'):
        S.cv_resize_batch(dev_sources, TARGET, 1, crop=CROP, out=torch.zeros(14, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match='image 1 must be'):
        S.cv_resize_batch([dev_sources[0], dev_sources[1].cpu()], TARGET, 1)
    with pytest.raises(ValueError, match='image 0 must be'):
        S.cv_resize_batch([dev_sources[2][:, ::2]], TARGET, 1)         # not contiguous
    with pytest.raises(ValueError, match='empty list'):
        S.cv_resize_batch([], TARGET, 1)
    assert S.cv_resize_batch_launches == before


def test_workload_shape_once():
    """the loop's shape: 375 x 500 and 512 x 512 to 256 x 256, centre crop 224; 512 x 512 is an exact 2 x 2 decimation, which LINEAR
    executes as AREA"""
    from robustart_amd.noise import imagenet_s as S
    arrs = [_noise(50, 375, 500), _noise(51, 512, 512)]
    dev = [torch.from_numpy(a).cuda() for a in arrs]
    crop = (16, 16, 224, 224)
    lin = area = None
    for f in INTERPS:
        got = S.cv_resize_batch(dev, (256, 256), f, crop=crop)
        want = [_oracle(a, (256, 256), f, crop) for a in arrs]
        assert not _bad(got, want), (f, _bad(got, want))
        lin, area = (got if f == 1 else lin), (got if f == 3 else area)
    assert torch.equal(lin[1], area[1]) and not torch.equal(lin[0], area[0])


PNG_SIZES = [(40, 60), (72, 72), (75, 100), (33, 47), (90, 64), (108, 72)]


@pytest.fixture(scope='module')
def png_folder(tmp_path_factory):
    root = tmp_path_factory.mktemp('cv_batch_folder')
    paths = []
    for k, (h, w) in enumerate(PNG_SIZES):
        p = root / ('img%02d.png' % k)
        Image.fromarray(_noise(200 + k, h, w)).save(str(p), 'PNG')
        paths.append(str(p))
    return paths


def test_image_transfer_batch_makes_one_call_per_operator(png_folder, monkeypatch):
    from robustart_amd.noise import imagenet_s as S
    singles, batches = [], []
    real_single, real_batch = S.cv_resize, S.cv_resize_batch
    decoded = [S.decode(p) for p in png_folder]
    for name in NAMES:
        # the expected bytes come from the per-image route, before the spies are in place
        want_val = [S.image_transfer(a, resize_type=name, transform_type='val', resize=32) for a in decoded]
        random.seed(11)
        boxes = [S._train_params(a.shape[:2], random) for a in decoded]
        want_train = [real_single(torch.from_numpy(np.ascontiguousarray(a[y:y + h, x:x + w])[None]).cuda(), (32, 32), S.CV_MODES[name])[0]
                      .cpu().numpy() for a, (y, x, h, w) in zip(decoded, boxes)]
        with monkeypatch.context() as m:
            m.setattr(S, 'cv_resize', lambda *a, **k: (singles.append(1), real_single(*a, **k))[1])
            m.setattr(S, 'cv_resize_batch', lambda *a, **k: (batches.append(1), real_batch(*a, **k))[1])
            got = S.image_transfer_batch(png_folder, resize_type=name, transform_type='val', resize=32)
            assert (len(singles), len(batches)) == (0, 1), name
            assert tuple(got.shape) == (6, 32, 32, 3) and not _bad(got, want_val), (name, _bad(got, want_val))
            random.seed(11)
            got = S.image_transfer_batch(png_folder, resize_type=name, transform_type='train', resize=32, decoded=decoded)
            assert (len(singles), len(batches)) == (0, 2), name
            assert not _bad(got, want_train), (name, _bad(got, want_train))
        del batches[:]
    assert len({tuple(b) for b in boxes}) > 1 and any(b[2:] != a.shape[:2] for a, b in zip(decoded, boxes))   # real boxes were drawn
