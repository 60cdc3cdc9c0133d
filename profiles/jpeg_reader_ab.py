"""FileImageNet.batch under ONECROP over 256 JPEG files, reader 'pil' against reader 'hip' -- the numbers of DESIGN.md 4.5.3.

    python profiles/jpeg_reader_ab.py [--images 256] [--reps 5] [--out profiles/jpeg_reader_ab.json]

Writes 256 JPEGs of 375 x 500 (4:2:0, quality 90, seeded smooth + noise content) into a temporary folder and times one batch() call
over all of them, a synchronize inside the timed region: 'pil' (the parent's path, the yardstick) and 'hip' at num_workers 1, 8 and 16,
the four variants alternating inside every repetition on one box; median of --reps repetitions after a warm-up round.  Also the split
of one hip batch (8 workers) into its host part (read + probe + entropy decode), the host-to-device copy and the device launches,
each followed by a synchronize.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_files(folder, n):
    import numpy as np
    from PIL import Image
    os.makedirs(os.path.join(folder, 'c0'))
    yy, xx = np.mgrid[0:375, 0:500].astype(np.float64)
    for k in range(n):
        rs = np.random.RandomState(k)
        base = np.stack([255 * xx / 499, 255 * yy / 374, 128 + 100 * np.sin(xx / (7.0 + k % 5) + yy / 5.0)], -1)
        arr = np.clip(base + rs.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(folder, 'c0', 'img%04d.jpg' % k), 'JPEG', quality=90, subsampling=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from robustart_amd.noise import imagenet_s
    from robustart_amd.train.cls_solver import FileImageNet
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    with tempfile.TemporaryDirectory() as folder:
        write_files(folder, a.images)
        size = sum(os.path.getsize(os.path.join(folder, 'c0', f)) for f in os.listdir(os.path.join(folder, 'c0')))
        sets = {'pil': FileImageNet.from_folder(folder, 224, 256, 'ONECROP', reader='pil')}
        for w in (1, 8, 16):
            sets['hip_w%d' % w] = FileImageNet.from_folder(folder, 224, 256, 'ONECROP', reader='hip', num_workers=w)
        idx = range(a.images)

        def once(ds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, _ = ds.batch(idx, 'cuda')
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        ref = once(sets['pil'])[1]
        times = {k: [] for k in sets}
        for rep in range(a.reps + 1):                      # round 0 is the warm-up
            for k, ds in sets.items():                     # the variants alternate inside a repetition
                t, out = once(ds)
                assert torch.equal(out, ref), k
                if rep:
                    times[k].append(t)
        res = {'images': a.images, 'image_hw': [375, 500], 'mean_file_bytes': size / a.images, 'reps': a.reps,
               'cpus_available': len(os.sched_getaffinity(0))}
        for k, ts in times.items():
            med = statistics.median(ts)
            res[k] = {'batch_ms': 1e3 * med, 'images_per_s': a.images / med, 'min_ms': 1e3 * min(ts), 'max_ms': 1e3 * max(ts)}
        for k in ('hip_w1', 'hip_w8', 'hip_w16'):
            res[k]['speedup_vs_pil'] = res['pil']['batch_ms'] / res[k]['batch_ms']
        assert sets['hip_w8'].decode_stats['fallback'] == 0
        paths = [os.path.join(folder, n) for n, _ in sets['pil'].items]
        splits = []
        for _ in range(a.reps):
            tm = {}
            imagenet_s.decode_batch_gpu(paths, 8, timings=tm)
            splits.append(tm)
        res['hip_w8_decode_split_ms'] = {k: 1e3 * statistics.median(s[k] for s in splits) for k in ('host_s', 'copy_s', 'device_s')}
        t0 = time.perf_counter()
        ds = sets['hip_w8']
        imgs = ds.decode_batch(idx, torch.device('cuda'))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        from robustart_amd.noise.imagenet_s import pil_resize
        for im in imgs:
            pil_resize(im[None], (256, 256), 1, crop=(16, 16, 224, 224))
        torch.cuda.synchronize()
        res['hip_w8_decode_ms'], res['hip_w8_resize_loop_ms'] = 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
