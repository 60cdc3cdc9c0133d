"""FileImageNet.batch under ONECROP over 256 JPEG files with reader 'hip': entropy decoding on host threads against entropy decoding
on the GPU -- the numbers of DESIGN.md 4.5.3, "Entropy decoding on the device".

    python profiles/jpeg_entropy_gpu_ab.py [--images 256] [--reps 5] [--out profiles/jpeg_entropy_gpu_ab.json]

The files are those of profiles/jpeg_reader_ab.py (375 x 500, 4:2:0, quality 90).  First the sweep that picks the default
subseq_bytes: the memset + kernel time of rart_jpeg_entropy_decode_gpu over the whole batch (device events) at 64 / 128 / 256 /
512 bytes, the sizes alternating inside every repetition, median of --reps after a warm-up round, rounds uncapped so that every
image converges; the A/B then runs at the fastest.  A/B: one batch() call over all files, a synchronize inside the timed region,
entropy='host' at 8 workers against entropy='gpu' at 8 workers and at 1 worker, outputs compared bit for bit first (with each other
and with the 'pil' reader), the variants alternating inside every repetition, median of --reps after a warm-up round.  Also the split
of one decode_batch_gpu call into its phases (timings: each phase followed by a synchronize) for the three variants.  Prints one
JSON object."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SWEEP = (64, 128, 256, 512)
UNCAPPED = 4097


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from jpeg_reader_ab import write_files
    from robustart_amd.noise import imagenet_s
    from robustart_amd.train.cls_solver import FileImageNet
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    with tempfile.TemporaryDirectory() as folder:
        write_files(folder, a.images)
        names = sorted(os.listdir(os.path.join(folder, 'c0')))
        paths = [os.path.join(folder, 'c0', f) for f in names]
        size = sum(os.path.getsize(p) for p in paths)
        res = {'images': a.images, 'image_hw': [375, 500], 'mean_file_bytes': size / a.images, 'reps': a.reps,
               'cpus_available': len(os.sched_getaffinity(0))}

        # the sweep: kernel time by subseq_bytes
        kernel = {s: [] for s in SWEEP}
        for rep in range(a.reps + 1):
            for s in SWEEP:
                before = dict(imagenet_s.entropy_stats)
                tm = {}
                imagenet_s.decode_batch_gpu(paths, 8, timings=tm, entropy='gpu', subseq_bytes=s, max_rounds=UNCAPPED)
                assert imagenet_s.entropy_stats['gpu'] - before['gpu'] == a.images
                if rep:
                    kernel[s].append(tm['entropy_kernel_s'])
        res['kernel_ms_by_subseq_bytes'] = {str(s): 1e3 * statistics.median(v) for s, v in kernel.items()}
        best = min(SWEEP, key=lambda s: statistics.median(kernel[s]))
        res['subseq_bytes'] = best
        imagenet_s.entropy_params['subseq_bytes'] = best
        imagenet_s.entropy_params['max_rounds'] = UNCAPPED

        # the rounds the batch needs at that size (the host emulation: the same count as the device's)
        import numpy as np
        rounds = []
        for p in paths[:32]:
            data = open(p, 'rb').read()
            info = imagenet_s.jpeg_probe(data)
            st, used = imagenet_s.jpeg_entropy_emulate(data, info, np.zeros(info.coef_count, np.int16), best, UNCAPPED)
            assert st == 0
            rounds.append(used)
        res['rounds_used_first_32_files'] = {'min': min(rounds), 'median': statistics.median(rounds), 'max': max(rounds)}

        sets = {'host_w8': FileImageNet.from_folder(folder, 224, 256, 'ONECROP', reader='hip', num_workers=8),
                'gpu_w8': FileImageNet.from_folder(folder, 224, 256, 'ONECROP', reader='hip', num_workers=8, entropy='gpu'),
                'gpu_w1': FileImageNet.from_folder(folder, 224, 256, 'ONECROP', reader='hip', num_workers=1, entropy='gpu')}
        idx = range(a.images)

        def once(ds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, _ = ds.batch(idx, 'cuda')
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        ref = FileImageNet.from_folder(folder, 224, 256, 'ONECROP', reader='pil').batch(idx, 'cuda')[0]
        for k, ds in sets.items():
            assert torch.equal(once(ds)[1], ref), k                # bit for bit, before any number is taken
        times = {k: [] for k in sets}
        for rep in range(a.reps + 1):                      # round 0 is the warm-up
            for k, ds in sets.items():                     # the variants alternate inside a repetition
                t, out = once(ds)
                assert torch.equal(out, ref), k
                if rep:
                    times[k].append(t)
        for k, ts in times.items():
            med = statistics.median(ts)
            res[k] = {'batch_ms': 1e3 * med, 'images_per_s': a.images / med, 'min_ms': 1e3 * min(ts), 'max_ms': 1e3 * max(ts)}
            assert sets[k].decode_stats['fallback'] == 0
        for k in ('gpu_w8', 'gpu_w1'):
            res[k]['speedup_vs_host_w8'] = res['host_w8']['batch_ms'] / res[k]['batch_ms']
        for k, (workers, mode) in {'host_w8': (8, 'host'), 'gpu_w8': (8, 'gpu'), 'gpu_w1': (1, 'gpu')}.items():
            splits = []
            for _ in range(a.reps):
                tm = {}
                imagenet_s.decode_batch_gpu(paths, workers, timings=tm, entropy=mode)
                splits.append(tm)
            res[k + '_decode_split_ms'] = {p: 1e3 * statistics.median(s[p] for s in splits) for p in sorted(splits[0])}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
