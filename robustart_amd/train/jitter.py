"""ColorJitter of a training batch: the config entry's ranges, the per-sample draws (host, pure) and the image operation (HIP).

Reference: the `ColorJitter` entry of the list-form `data.train.transforms` of exprs/exp/imagenet_s_loop/config_{convnext_base,
convnextv2_base, vit_base, convnext_base_cvst, vit_base_cvst}.yaml:67-72 (brightness 0.2, contrast 0.2, saturation 0.2, hue 0.1).
torchvision, which interprets the entry, is not part of this build; how it composes the operations is restated here and is UNPINNED
(DESIGN 4.5.2).  What each operation computes on a PIL image is Pillow's arithmetic, and that is pinned: rart_color_jitter_u8 returns
Pillow's bytes.
  per sample: a permutation of (0 brightness, 1 contrast, 2 saturation, 3 hue) gives the order; an operation whose range is degenerate is
  skipped in whatever position it has; brightness / contrast / saturation factor f ~ U(max(0, 1 - v), 1 + v), hue factor f ~ U(-h, h),
  applied as the uint8 shift int(f * 255) & 255 of the H plane.
torchvision's own random stream is not reproduced: every draw of sample `index` in `epoch` comes from a numpy Generator keyed by
(data.seed, epoch, index) alone, like FileImageNet.box -- resume-safe and the same for every world size.

    ranges = jitter_ranges({'brightness': 0.2, 'contrast': 0.2, 'saturation': 0.2, 'hue': 0.1})    # four (lo, hi) or None each; or None
    plan = draw_jitter(ranges, seed, epoch, index)                                                  # (order, b, c, s, hue_factor)
    apply_jitter(batch_u8, [plan, ...])                                                             # HIP: rart_color_jitter_u8, in place
"""
import ctypes
import numbers

import numpy as np
import torch

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
KEYS = ('brightness', 'contrast', 'saturation', 'hue')
SKIP = 255                    # an operation id the kernel skips
_STREAM = 0x6A6974            # 'jit': keeps these draws apart from any other generator seeded by (seed, epoch, index)


def _check_range(name, value, center, bound, clip_first_on_zero):
    """torchvision's ColorJitter._check_input: a number v -> [center - v, center + v] (the lower end clipped at 0 for the blend factors), a
    pair as it is; lo <= hi inside `bound`; None when the range is the neutral value alone."""
    if isinstance(value, bool):
        raise ValueError('ColorJitter %s: a number or a pair [lo, hi], got %r' % (name, value))
    if isinstance(value, numbers.Number):
        if not value >= 0:
            raise ValueError('ColorJitter %s: a single number must be non negative, got %r' % (name, value))
        lo, hi = center - float(value), center + float(value)
        if clip_first_on_zero:
            lo = max(lo, 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2 and all(isinstance(v, numbers.Number) and not isinstance(v, bool) for v in value):
        lo, hi = float(value[0]), float(value[1])
    else:
        raise ValueError('ColorJitter %s: a number or a pair [lo, hi], got %r' % (name, value))
    if not bound[0] <= lo <= hi <= bound[1]:
        raise ValueError('ColorJitter %s: values must satisfy %g <= lo <= hi <= %g, got [%r, %r]' % (name, bound[0], bound[1], lo, hi))
    return None if lo == hi == center else (lo, hi)


def jitter_ranges(kwargs):
    """-> ((lo, hi) or None for brightness, contrast, saturation, hue) from the entry's kwargs, or None when no operation is active (an
    absent entry, no kwargs, or only neutral values).  Raises ValueError naming the key, as torchvision validates."""
    kwargs = dict(kwargs or {})
    unknown = sorted(set(kwargs) - set(KEYS))
    if unknown:
        raise ValueError('ColorJitter: unknown kwargs %s (brightness, contrast, saturation, hue)' % unknown)
    out = []
    for name in KEYS:
        v = kwargs.get(name)
        v = 0 if v is None else v
        if name == 'hue':
            out.append(_check_range(name, v, 0.0, (-0.5, 0.5), False))
        else:
            out.append(_check_range(name, v, 1.0, (0.0, float('inf')), True))
    return tuple(out) if any(r is not None for r in out) else None


def draw_jitter(ranges, seed, epoch, index):
    """The plan of sample `index` (global) in `epoch`: (order, b, c, s, hue_factor) -- order a tuple, a permutation of (0, 1, 2, 3); a
    factor is a Python float, or None where the operation's range is None.  The permutation is drawn first, then the factors of the active
    operations in the fixed order b, c, s, h.  A pure function of its arguments."""
    g = np.random.default_rng([_STREAM, int(seed), int(epoch), int(index)])
    order = tuple(int(v) for v in g.permutation(4))
    return (order,) + tuple(None if r is None else float(g.uniform(r[0], r[1])) for r in ranges)


def hue_shift(hue_factor):
    """the uint8 added to the H plane: int() truncates toward zero and the cast wraps (0.1 -> 25, -0.1 -> 231)"""
    return int(hue_factor * 255) & 255


def pack_jitter(plans):
    """plans -> a uint8 numpy array [n, 20], the rart_jitter_rec records of include/robustart_hip.h (ids in application order with SKIP for
    an inactive operation, the three blend factors as fp32, the hue shift).  A plan is (order, b, c, s, hue_factor) with None for an
    inactive operation, or None for a sample that is copied.  The kernel cannot refuse a bad record, so everything is validated here."""
    from .. import _lib
    recs = (_lib.JitterRec * len(plans))()
    for k, plan in enumerate(plans):
        rec = recs[k]
        rec.op[:] = [SKIP] * 4
        if plan is None:
            continue
        order, b, c, s, hf = plan
        order = [int(o) for o in order]
        if len(order) > 4 or any(o < 0 or o > 3 for o in order) or len(set(order)) != len(order):
            raise ValueError('pack_jitter: sample %d: order must hold distinct operation ids in 0..3, got %r' % (k, order))
        for name, f in zip(KEYS[:3], (b, c, s)):
            if f is not None and not (0.0 <= float(f) < float('inf')):
                raise ValueError('pack_jitter: sample %d: the %s factor must be finite and non negative, got %r' % (k, name, f))
        if hf is not None and not (-0.5 <= float(hf) <= 0.5):
            raise ValueError('pack_jitter: sample %d: the hue factor must lie in [-0.5, 0.5], got %r' % (k, hf))
        active = (b, c, s, hf)
        for slot, o in enumerate(order):
            rec.op[slot] = o if active[o] is not None else SKIP
        for i, f in enumerate((b, c, s)):
            rec.factor[i] = 0.0 if f is None else float(f)
        rec.hue_shift = 0 if hf is None else hue_shift(float(hf))
    assert ctypes.sizeof(_lib.JitterRec) == 20
    return np.frombuffer(bytes(recs), dtype=np.uint8).reshape(len(plans), 20).copy()


def apply_jitter(batch, plans, out=None):
    """ColorJitter of a uint8 NHWC batch [B, H, W, 3] on the GPU through rart_color_jitter_u8: one call for the whole batch, in place
    (out=None; `batch` is returned) or into `out`, a tensor of the same shape that does not overlap it.  plans: B plans (pack_jitter).  The
    records leave from pinned memory; nothing is read back from the device.  There is no CPU fallback: a CPU tensor raises."""
    from .. import _lib
    if batch.device.type != 'cuda':
        raise RuntimeError('apply_jitter runs on the GPU (rart_color_jitter_u8); there is no CPU fallback')
    if batch.dim() != 4 or batch.dtype != torch.uint8 or batch.shape[3] != 3 or not batch.is_contiguous():
        raise ValueError('apply_jitter: the batch must be contiguous u8 [B, H, W, 3], got %s %s' % (batch.dtype, tuple(batch.shape)))
    B, H, W = int(batch.shape[0]), int(batch.shape[1]), int(batch.shape[2])
    if len(plans) != B:
        raise ValueError('apply_jitter: %d plans for a batch of %d' % (len(plans), B))
    if out is None:
        out = batch
    elif out.device != batch.device or out.dtype != torch.uint8 or out.shape != batch.shape or not out.is_contiguous():
        raise ValueError('apply_jitter: out must be a contiguous u8 tensor of the batch\'s shape on its device')
    if B == 0:
        return out
    recs = torch.from_numpy(pack_jitter(plans)).pin_memory().to(batch.device, non_blocking=True)
    lsum = torch.empty(B, dtype=torch.int32, device=batch.device)
    _lib.check(_lib.load().rart_color_jitter_u8(_lib.ptr(batch), _lib.ptr(out), B, H, W, _lib.ptr(recs), _lib.ptr(lsum), _lib.stream_ptr()))
    return out
