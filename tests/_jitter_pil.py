"""The expected value of the ColorJitter tests: torchvision's ColorJitter on a PIL image, restated as the Pillow calls it consists of.
torchvision.transforms.functional on a PIL image is adjust_brightness / adjust_contrast / adjust_saturation = ImageEnhance.Brightness /
Contrast / Color(img).enhance(f) and adjust_hue = convert('HSV'), a uint8 wrap-around add on the H plane, convert('RGB').  A test helper:
the product never imports it."""
import numpy as np
from PIL import Image, ImageEnhance

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def hue_shift(hue_factor):
    """the uint8 that torchvision adds to the H plane: int() truncates toward zero, the cast wraps"""
    return int(hue_factor * 255) & 255


def shift_hue(img, shift):
    """adjust_hue with the shift given as the uint8 itself; the HSV round trip runs at shift 0 too"""
    h, s, v = img.convert('HSV').split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over='ignore'):
        np_h += np.uint8(shift)
    return Image.merge('HSV', (Image.fromarray(np_h, 'L'), s, v)).convert('RGB')


def jitter_pil(arr, order, b=None, c=None, s=None, shift=None):
    """arr: uint8 [h, w, 3].  order: operation ids in application order; an operation whose argument is None (or an id outside 0..3) is
    skipped in whatever position it has.  b, c, s: the enhance factors; shift: the uint8 hue shift.  -> uint8 [h, w, 3]"""
    img = Image.fromarray(np.ascontiguousarray(arr), 'RGB')
    for op in order:
        if op == BRIGHTNESS and b is not None:
            img = ImageEnhance.Brightness(img).enhance(b)
        elif op == CONTRAST and c is not None:
            img = ImageEnhance.Contrast(img).enhance(c)
        elif op == SATURATION and s is not None:
            img = ImageEnhance.Color(img).enhance(s)
        elif op == HUE and shift is not None:
            img = shift_hue(img, shift)
    return np.array(img, dtype=np.uint8)


def jitter_pil_plan(arr, plan):
    """plan: what robustart_amd.train.jitter.draw_jitter returns, (order, b, c, s, hue_factor)"""
    order, b, c, s, hf = plan
    return jitter_pil(arr, order, b, c, s, None if hf is None else hue_shift(hf))
