"""Mixup / CutMix of a training batch on the GPU, the numbers of DESIGN.md 4.5.1: rart_mix_batch_f32 at B = 256, 224 x 224 against the torch
expression chain it replaces (permute / float / div, index, two multiplies, add; for CutMix: permute / float / div, clone, index, slice
assignment) on the same tensors; for an fp32 source the chain has no permute / float / div step.  CUDA events around `--reps` back-to-back
launches (20 warm-up calls), median of `--windows` windows; the slower torch chain is timed with `--reps` / 4 calls per window after 5
warm-up calls.

    python profiles/mix_batch_time.py [--batch 256] [--size 224] [--out result.json]

Prints one JSON object.  Per case: microseconds per call of the launch and of the torch chain, the launch's algorithmic bytes (what the
operation has to read and write, from the shapes), the time those bytes take at 8 TB/s, and both measured times over that bound."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12


def algorithmic_bytes(kind, is_u8, B, H, W):
    """bytes the operation must move: every output element written once (fp32), every needed source element read once"""
    px = H * W
    src_img = 3 * px * (1 if is_u8 else 4)
    if kind == 'mixup':
        read = 2 * src_img                                   # the own image and the partner
    else:
        read = src_img                                       # each pixel from exactly one of the two
    return B * (read + 12 * px)


def timed(torch, fn, reps, windows, warm=20):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from robustart_amd import _lib as L
    from robustart_amd.train.mixing import apply_mix_torch, cutmix_box
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    B, H, W = a.batch, a.size, a.size
    lib = L.load()
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    f32 = u8.permute(0, 3, 1, 2).float().div(255.0).contiguous()
    perm = np.random.default_rng(0).permutation(B)
    perm_dev = torch.from_numpy(perm.astype(np.int32)).cuda()
    idx = torch.from_numpy(perm.astype(np.int64)).cuda()
    dst = torch.empty(B, 3, H, W, device='cuda')
    box, lam_box = cutmix_box(0.5, H // 2, W // 2, H, W)      # the mean box of alpha = 1: half the pixels
    res = {'batch': B, 'size': H, 'reps': a.reps, 'windows': a.windows, 'cutmix_box': list(box), 'hbm_bytes_per_s': HBM_BYTES_PER_S}
    for kind, plan in (('mixup', ('mixup', 0.2871, perm, None)), ('cutmix', ('cutmix', lam_box, perm, box))):
        for is_u8, src in ((True, u8), (False, f32)):
            y0, y1, x0, x1 = box if kind == 'cutmix' else (0, 0, 0, 0)

            def launch():
                L.check(lib.rart_mix_batch_f32(src.data_ptr(), 1 if is_u8 else 0, perm_dev.data_ptr(), dst.data_ptr(), B, H, W,
                                               1 if kind == 'mixup' else 2, plan[1], y0, y1, x0, x1, L.stream_ptr()))
            launch()
            assert torch.equal(dst, apply_mix_torch(src, plan)), (kind, is_u8)        # the timed launch computes the chain's result
            hip = timed(torch, launch, a.reps, a.windows)

            def chain():                                     # the index tensor is on the device already, as perm_dev is for the launch
                x01 = src.permute(0, 3, 1, 2).float().div(255.0) if is_u8 else src
                if kind == 'mixup':
                    return plan[1] * x01 + (1.0 - plan[1]) * x01[idx]
                out = x01.clone(memory_format=torch.contiguous_format)
                out[:, :, y0:y1, x0:x1] = x01[idx][:, :, y0:y1, x0:x1]
                return out
            assert torch.equal(dst, chain())
            ref = timed(torch, chain, max(a.reps // 4, 1), a.windows, warm=5)
            nbytes = algorithmic_bytes(kind, is_u8, B, H, W)
            bound_us = nbytes / HBM_BYTES_PER_S * 1e6
            res['%s_%s' % (kind, 'u8' if is_u8 else 'f32')] = {
                'launch_us': hip[0], 'launch_us_min_max': [hip[1], hip[2]], 'torch_chain_us': ref[0], 'torch_chain_us_min_max': [ref[1], ref[2]],
                'algorithmic_bytes': nbytes, 'bytes_over_8TBps_us': bound_us, 'launch_over_bound': hip[0] / bound_us,
                'torch_chain_over_bound': ref[0] / bound_us, 'launch_TBps': nbytes / hip[0] * 1e-6}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
