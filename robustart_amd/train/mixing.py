"""Mixup / CutMix of a training batch: the config keys, the per-iteration draws (host, pure) and the image operation.

Reference: the keys `mixup: 0.2` / `cutmix: 1.0` of exprs/nips_benchmark/augmentation/{resnet50, vit_base_patch16_224, mixer_B16_224}/
config.yaml:30-31 (every other config carries them commented out).  The solver that reads them (`prototype...cls_solver`) is absent, so
the behaviour is restated from the published recipes it wraps and is UNPINNED:
  Mixup  (Zhang et al., ICLR 2018): lam ~ Beta(a, a), x = lam * x + (1 - lam) * x[perm], loss = lam * L(y) + (1 - lam) * L(y[perm]);
  CutMix (Yun et al., ICCV 2019):   lam0 ~ Beta(a, a), a box of area ratio 1 - lam0 around a uniform centre, clipped to the image, is
                                    pasted from x[perm]; lam = 1 - the clipped box's exact area ratio weighs the two losses.
With both keys active an iteration applies exactly ONE of the two, chosen with probability 1/2.

Every draw of iteration `it` on rank `rank` comes from a numpy Generator keyed by (data.seed, it, rank) alone: no state is carried from
one iteration to the next, so a resumed run repeats the draws of an uninterrupted one.

    plan = draw_mix(mixup, cutmix, seed, it, rank, B, H, W)        # (kind, lam, perm, box) or None
    x01 = apply_mix(imgs, plan, device)                            # HIP: rart_mix_batch_f32, u8 NHWC or fp32 NCHW -> fp32 NCHW
    x01 = apply_mix_torch(imgs, plan)                              # the same expressions in torch (CPU / --engine torch scaffold)
"""
import math

import numpy as np
import torch

MIXUP, CUTMIX = 'mixup', 'cutmix'
_MODE = {MIXUP: 1, CUTMIX: 2}
_STREAM = 0x6D6978            # 'mix': keeps these draws apart from any other generator seeded by (seed, it, rank)


def mix_alphas(cfg):
    """-> (mixup alpha or None, cutmix alpha or None) from the solver's config.  `mixup` is active for 0 < value < 1 (the reference's
    default 1.0 means off), `cutmix` for value > 0; an absent key (or null) is off."""
    m, c = cfg.get('mixup'), cfg.get('cutmix')
    m = float(m) if m is not None else None
    c = float(c) if c is not None else None
    return (m if m is not None and 0.0 < m < 1.0 else None), (c if c is not None and c > 0.0 else None)


def cutmix_box(lam0, cy, cx, H, W):
    """-> ((y0, y1, x0, x1), lam): the box of area ratio 1 - lam0 centred at (cy, cx), clipped to the H x W image, and the weight of the
    own image, 1 - the clipped box's exact share of the pixels."""
    r = math.sqrt(1.0 - float(lam0))
    ch, cw = int(H * r), int(W * r)
    clip = lambda v, hi: max(0, min(int(v), hi))      # noqa: E731
    y0, y1 = clip(cy - ch // 2, H), clip(cy + ch // 2, H)
    x0, x1 = clip(cx - cw // 2, W), clip(cx + cw // 2, W)
    return (y0, y1, x0, x1), 1.0 - (y1 - y0) * (x1 - x0) / float(H * W)


def draw_mix(mixup, cutmix, seed, it, rank, B, H, W):
    """The plan of iteration `it` on rank `rank`: (kind, lam, perm, box) -- kind 'mixup' / 'cutmix', lam a Python float, perm an int64
    numpy permutation of B, box (y0, y1, x0, x1) (None for Mixup) -- or None when neither alpha is given.  mixup / cutmix: the Beta
    parameter of the operation or None (see mix_alphas).  A pure function of its arguments."""
    if mixup is None and cutmix is None:
        return None
    g = np.random.default_rng([_STREAM, int(seed), int(it), int(rank)])
    if mixup is not None and cutmix is not None:
        kind = MIXUP if g.random() < 0.5 else CUTMIX
    else:
        kind = MIXUP if mixup is not None else CUTMIX
    if kind == MIXUP:
        lam = float(g.beta(mixup, mixup))
        return kind, lam, g.permutation(int(B)), None
    lam0 = float(g.beta(cutmix, cutmix))
    cy, cx = int(g.integers(0, int(H))), int(g.integers(0, int(W)))
    perm = g.permutation(int(B))
    box, lam = cutmix_box(lam0, cy, cx, int(H), int(W))
    return kind, lam, perm, box


def _geometry(src):
    """-> (is_u8, B, H, W) of a u8 NHWC or fp32 NCHW batch"""
    if src.dim() != 4:
        raise ValueError('apply_mix: the batch must be u8 [B, H, W, 3] or fp32 [B, 3, H, W], got %s' % (tuple(src.shape),))
    if src.dtype == torch.uint8 and src.shape[3] == 3:
        return True, int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    if src.dtype == torch.float32 and src.shape[1] == 3:
        return False, int(src.shape[0]), int(src.shape[2]), int(src.shape[3])
    raise ValueError('apply_mix: the batch must be u8 [B, H, W, 3] or fp32 [B, 3, H, W], got %s %s' % (src.dtype, tuple(src.shape)))


def _checked_perm(perm, B):
    perm = np.asarray(perm)
    if perm.shape != (B,) or perm.min() < 0 or perm.max() >= B:
        raise ValueError('apply_mix: perm must hold %d indices in [0, %d)' % (B, B))
    return perm


def upload_perm(plan, B, device):
    """plan's permutation as an int32 tensor on `device`; its range is checked here, on the host (the kernel trusts it).  For a GPU the copy
    leaves from pinned memory and does not block the host (the host allocator keeps the staging block until the copy has run)."""
    perm = torch.from_numpy(_checked_perm(plan[2], int(B)).astype(np.int32))
    if torch.device(device).type == 'cuda':
        return perm.pin_memory().to(device, non_blocking=True)
    return perm.to(device)


def apply_mix(src, plan, device=None, perm_dev=None):
    """The mixed batch as fp32 NCHW in [0, 1] through rart_mix_batch_f32 (one launch, fusing the u8 -> [0, 1] hand-over).  src: u8 NHWC as
    the datasets hand it over, or fp32 NCHW in [0, 1], on the GPU.  `perm` is uploaded once as int32 (upload_perm; a caller that needs the
    device copy too, for the partner labels, passes its own as perm_dev); nothing is read back from the device."""
    from .. import _lib
    kind, lam, perm, box = plan
    device = torch.device(device) if device is not None else src.device
    if device.type != 'cuda' or src.device.type != 'cuda':
        raise RuntimeError('apply_mix runs on the GPU (rart_mix_batch_f32); apply_mix_torch is the CPU scaffold')
    is_u8, B, H, W = _geometry(src)
    src = src.contiguous()
    if perm_dev is None:
        perm_dev = upload_perm(plan, B, device)
    elif perm_dev.dtype != torch.int32 or perm_dev.shape != (B,) or perm_dev.device.type != 'cuda' or not perm_dev.is_contiguous():
        raise ValueError('apply_mix: perm_dev must be the contiguous int32 [%d] device copy of the plan\'s perm (upload_perm)' % B)
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=device)
    y0, y1, x0, x1 = box if box is not None else (0, 0, 0, 0)
    _lib.check(_lib.load().rart_mix_batch_f32(_lib.ptr(src), 1 if is_u8 else 0, _lib.ptr(perm_dev), _lib.ptr(out), B, H, W, _MODE[kind],
                                              float(lam), int(y0), int(y1), int(x0), int(x1), _lib.stream_ptr()))
    return out


def apply_mix_torch(src, plan):
    """apply_mix restated in torch on src's device: the expression chain the HIP launch replaces."""
    kind, lam, perm, box = plan
    is_u8, B, H, W = _geometry(src)
    x01 = src.permute(0, 3, 1, 2).float().div(255.0) if is_u8 else src
    idx = torch.from_numpy(_checked_perm(perm, B).astype(np.int64)).to(src.device)
    if kind == MIXUP:
        return lam * x01 + (1.0 - lam) * x01[idx]
    y0, y1, x0, x1 = box
    out = x01.clone(memory_format=torch.contiguous_format)
    out[:, :, y0:y1, x0:x1] = x01[idx][:, :, y0:y1, x0:x1]
    return out
