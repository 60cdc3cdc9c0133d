"""ColorJitter of a training batch on the GPU, the numbers of DESIGN.md 4.5.2: rart_color_jitter_u8 at B = 256, 224 x 224 with all four
operations active (the reference configs' ranges, one drawn plan per sample), from one buffer into another so that every call sees the
same pixels (in place, as FileImageNet.batch calls it, moves the same bytes).  CUDA events around
`--reps` back-to-back calls (20 warm-up calls), median of `--windows` windows.  For scale, the host time of the Pillow calls the launch
replaces for the same 256 images and plans (one pass, one process), and the same entry with the plans that have no contrast (the first
launch then only reads the records).

    python profiles/color_jitter_time.py [--batch 256] [--size 224] [--out result.json]

Prints one JSON object: microseconds per call, the bytes the two-launch form moves (two reads and one write of the batch), the time those
bytes take at the best plain copy this project has measured (0.65 of 8 TB/s), and the measured time over that bound."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HBM_BYTES_PER_S = 8.0e12
BEST_COPY_FRACTION = 0.65


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
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from _jitter_pil import jitter_pil_plan               # the Pillow composition the tests compare against
    from robustart_amd import _lib as L
    from robustart_amd.train.jitter import draw_jitter, jitter_ranges, pack_jitter
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    B, H, W = a.batch, a.size, a.size
    lib = L.load()
    host = np.random.RandomState(0).randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    src = torch.from_numpy(host).cuda()
    work = torch.empty_like(src)
    lsum = torch.empty(B, dtype=torch.int32, device='cuda')
    ranges = jitter_ranges({'brightness': 0.2, 'contrast': 0.2, 'saturation': 0.2, 'hue': 0.1})
    plans = [draw_jitter(ranges, 0, 0, i) for i in range(B)]
    no_contrast = [(o, b, None, s, h) for o, b, c, s, h in plans]
    t0 = time.perf_counter()
    want = np.stack([jitter_pil_plan(host[i], plans[i]) for i in range(B)])
    pillow_s = time.perf_counter() - t0
    res = {'batch': B, 'size': H, 'reps': a.reps, 'windows': a.windows, 'hbm_bytes_per_s': HBM_BYTES_PER_S,
           'best_copy_fraction': BEST_COPY_FRACTION, 'host_pillow_ms_for_the_batch': pillow_s * 1e3}
    for name, pl, passes in (('all_four', plans, 3), ('no_contrast', no_contrast, 2)):
        nbytes = passes * B * H * W * 3                    # two reads and one write of the batch; without a contrast slot, one read
        bound_us = nbytes / (BEST_COPY_FRACTION * HBM_BYTES_PER_S) * 1e6
        recs = torch.from_numpy(pack_jitter(pl)).cuda()

        def launch():
            L.check(lib.rart_color_jitter_u8(src.data_ptr(), work.data_ptr(), B, H, W, recs.data_ptr(), lsum.data_ptr(), L.stream_ptr()))
        if name == 'all_four':                             # the timed launch computes Pillow's bytes
            launch()
            assert np.array_equal(work.cpu().numpy(), want)
        us = timed(torch, launch, a.reps, a.windows)
        res[name] = {'launch_us': us[0], 'launch_us_min_max': [us[1], us[2]], 'bytes_moved': nbytes, 'bytes_at_best_copy_us': bound_us,
                     'launch_over_bound': us[0] / bound_us, 'fraction_of_best_copy': bound_us / us[0], 'TBps': nbytes / us[0] * 1e-6,
                     'pillow_over_launch': pillow_s * 1e6 / us[0]}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
