"""Reference statements for the batched variable-size resize, in Pillow only: crop(box) -> resize -> crop window -> mirror, and the
shared sources of tests/test_resize_batch_gpu.py."""
import functools

import numpy as np
from PIL import Image

from _inputs import make_image

# the library's filter ids 0..5 (noise.imagenet_s.PIL_FILTERS) -> Pillow's constants
PIL_ID = {0: Image.NEAREST, 1: Image.BILINEAR, 2: Image.BICUBIC, 3: Image.BOX, 4: Image.HAMMING, 5: Image.LANCZOS}

# a source narrower than the support, up- and down-scaling in one image, 151 taps (900 -> 36, LANCZOS), the identity (36 x 36) and
# first-pass work that differs by more than 100 x between neighbours
SIZES = [(1, 1), (2, 3), (37, 1000), (900, 700), (75, 100), (36, 36), (33, 47), (400, 9)]


@functools.lru_cache(maxsize=None)
def sources():
    out = tuple(make_image(k, h, w) for k, (h, w) in enumerate(SIZES))
    for a in out:
        a.setflags(write=False)
    return out


def pillow(x, resize_hw, f, crop=None, box=None, flip=False):
    """x: HxWx3 uint8; box (y, x, h, w) or None; crop (cy, cx, ch, cw) or None -> the uint8 array Pillow gives"""
    img = Image.fromarray(np.ascontiguousarray(x))
    if box is not None:
        y, x0, h, w = box
        img = img.crop((x0, y, x0 + w, y + h))
    img = img.resize((int(resize_hw[1]), int(resize_hw[0])), PIL_ID[f])
    if crop is not None:
        cy, cx, ch, cw = crop
        img = img.crop((cx, cy, cx + cw, cy + ch))
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(img)


def pillow_box_argument(x, resize_hw, f, box):
    """Image.resize(box=...): the OTHER reading of a box, which lets the filter support read source pixels outside it"""
    y, x0, h, w = box
    return np.asarray(Image.fromarray(np.ascontiguousarray(x)).resize((int(resize_hw[1]), int(resize_hw[0])), PIL_ID[f],
                                                                      box=(x0, y, x0 + w, y + h)))


@functools.lru_cache(maxsize=None)
def expected(resize_hw, f, crop, boxes=None, flips=None):
    """Pillow's result for every source of sources(); boxes / flips: tuples per image or None"""
    return tuple(pillow(x, resize_hw, f, crop, None if boxes is None else boxes[k], bool(flips[k]) if flips is not None else False)
                 for k, x in enumerate(sources()))
