"""Subset confidence on the GPU, the numbers of DESIGN.md 4.8: rart_logit_confidence_f32 at rows = 256, classes = 1000, K = 200 (one
evaluation batch of the imagenet-a_o-loop configs' models) beside the torch expression it replaces,
`softmax(logits[:, idx], 1).max(1)`, on the same tensor.  Both are timed in one process, in alternating windows: CUDA events around
`--reps` back-to-back calls (50 warm-up calls), median / min / max of `--windows` windows.  At this size both are a few microseconds of
device work, so a window of back-to-back calls measures the rate at which the host can enqueue them as much as the kernels; the kernel
times themselves come from running this script under `rocprofv3 --kernel-trace --stats` (its own run, fewer reps).

    python profiles/logit_confidence_time.py [--rows 256] [--classes 1000] [--k 200] [--out result.json]

Prints one JSON object: microseconds per call of the two forms, the launches each form makes, and the largest difference of their results."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=256)
    ap.add_argument('--classes', type=int, default=1000)
    ap.add_argument('--k', type=int, default=200)
    ap.add_argument('--reps', type=int, default=2000)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from robustart_amd.metrics import class_subset, subset_confidence
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    rs = np.random.RandomState(0)
    logits = torch.from_numpy(rs.standard_normal((a.rows, a.classes)).astype(np.float32) * 4).cuda()
    idx = sorted(rs.choice(a.classes, a.k, replace=False).tolist())
    sub = class_subset(idx, a.classes, 'cuda')
    idx_long = sub.long()
    labels = torch.from_numpy(rs.randint(0, a.k, a.rows)).cuda()

    def hip():
        return subset_confidence(logits, sub, labels)

    def torch_form():
        conf, pred = torch.softmax(logits[:, idx_long], 1).max(1)
        return pred, conf, pred == labels

    p0, c0, k0 = hip()
    p1, c1, k1 = torch_form()
    assert torch.equal(p0.long(), p1) and torch.equal(k0.bool(), k1)
    diff = float(((c0 - c1).abs() / c1).max())
    for _ in range(50):
        hip()
        torch_form()
    t = {'hip': [], 'torch': []}
    for _ in range(a.windows):                       # alternate, so that a drift of the clock or the host meets both forms alike
        t['hip'].append(window(torch, hip, a.reps))
        t['torch'].append(window(torch, torch_form, a.reps))
    out = {'rows': a.rows, 'classes': a.classes, 'k': a.k, 'reps': a.reps, 'windows': a.windows,
           'hip_us_per_call': {'median': statistics.median(t['hip']), 'min': min(t['hip']), 'max': max(t['hip'])},
           'torch_us_per_call': {'median': statistics.median(t['torch']), 'min': min(t['torch']), 'max': max(t['torch'])},
           'hip_launches_per_call': 1, 'torch_expression': 'softmax(logits[:, idx], 1).max(1); pred == labels',
           'max_rel_diff_of_conf': diff, 'device': torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
