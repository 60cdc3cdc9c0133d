"""The ImageNet-C loop against the only way to score the same pairs before it, the numbers of DESIGN.md 4.10.

1. Whole loop: 256 JPEG files of 375 x 500 written from a seed, `image_reader.type: hip`, ResNet-50 on the bf16 engine, one batch of
   256.  `--evaluate --imagenet-c` over the 15 standard corruptions x 5 severities (frost photographs from a folder of seeded
   arrays) beside 75 `--evaluate --corruption NAME --severity S` calls of evaluate() in the same process, the torch module built
   once and passed in.  The two are alternated `--rounds` times after one warm-up of each; a host clock around calls that end in a
   read of the counters.  The per-pair hit counts of the two forms are compared.
2. The scoring step alone at 256 x 1000: cls_solver.topk_correct (torch.topk and two reads) beside metrics.topk_score adding to
   device counters, in alternating windows of back-to-back calls.

    python profiles/imagenet_c_loop_ab.py [--files 256] [--rounds 3] [--out result.json]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Args:
    engine = 'hip'
    corruption = None
    attack = None
    eps = '8/255'
    steps = 0
    severity = 3
    seed = 0
    precision = 'bf16'
    save_dir = None
    src_name = None
    tgt_name = None
    tgt_type = None
    imagenet_c = False
    imagenet_c_names = None
    imagenet_c_severities = None
    imagenet_c_frost_dir = None
    imagenet_c_scores = False


def write_files(root, n):
    import numpy as np
    from PIL import Image
    rs = np.random.RandomState(0)
    os.makedirs(os.path.join(root, 'val'))
    os.makedirs(os.path.join(root, 'frost'))
    yy, xx = np.mgrid[0:375, 0:500]
    lines = []
    for i in range(n):
        base = np.stack([127 + 100 * np.sin(xx / (9.0 + i % 17)) * np.cos(yy / 17.0), 127 + 90 * np.cos(xx / 23.0 + i),
                         127 + 80 * np.sin((xx + yy) / (11.0 + i % 13))], -1)
        arr = np.clip(base + rs.randn(375, 500, 3) * 12, 0, 255).astype(np.uint8)
        name = 'img_%03d.jpg' % i
        Image.fromarray(arr).save(os.path.join(root, 'val', name), quality=90)
        lines.append(json.dumps({'filename': name, 'label': (i * 37) % 1000}))
    with open(os.path.join(root, 'meta.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    for k in range(6):
        Image.fromarray(rs.randint(0, 256, (300, 320, 3)).astype(np.uint8)).save(os.path.join(root, 'frost', 'frost%d.png' % (k + 1)))


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=500)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from robustart_amd.metrics import topk_score
    from robustart_amd.model import get_model
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    from robustart_amd.noise import imagenet_c as C
    from robustart_amd.train import cls_solver as S
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    root = tempfile.mkdtemp()
    write_files(root, a.files)
    cfg = {'model': {'type': 'resnet50_official'},
           'data': {'type': 'imagenet', 'read_from': 'fs', 'batch_size': 256, 'input_size': 224, 'test_resize': 256, 'num_workers': 8,
                    'test': {'root_dir': os.path.join(root, 'val'), 'meta_file': os.path.join(root, 'meta.txt'),
                             'image_reader': {'type': 'hip'}, 'transforms': {'type': 'ONECROP'},
                             'imagenet_c_frost_dir': os.path.join(root, 'frost')}}}
    torch.manual_seed(0)
    model = randomize_bn_stats(get_model(cfg['model'])).eval()
    rank, world, device = S.init_dist()
    names = list(C.CORRUPTION_NAMES[:15])
    pairs = [(c, s) for c in names for s in (1, 2, 3, 4, 5)]

    def loop():
        x = Args()
        x.imagenet_c = True
        t0 = time.perf_counter()
        res = quiet(S.evaluate, cfg, x, rank, world, device, model=model)
        torch.cuda.synchronize()
        n = res['count']
        return time.perf_counter() - t0, {p: (round(res['imagenet_c']['%s/%d' % p]['top1'] * n / 100),
                                              round(res['imagenet_c']['%s/%d' % p]['top5'] * n / 100)) for p in pairs}

    def calls():
        counts = {}
        t0 = time.perf_counter()
        for c, s in pairs:
            x = Args()
            x.corruption, x.severity = c, s
            res = quiet(S.evaluate, cfg, x, rank, world, device, model=model)
            counts[(c, s)] = (round(res['top1'] * res['count']), round(res['top5'] * res['count']))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, counts

    loop()                                            # warm-up of each form: code objects, the reader's threads, the allocator
    calls()
    t_loop, t_calls, differing = [], [], 0
    for _ in range(a.rounds):                         # alternate, so that a drift of the clock or the host meets both forms alike
        tl, cl = loop()
        tc, cc = calls()
        t_loop.append(tl)
        t_calls.append(tc)
        differing += sum(1 for p in pairs if cl[p] != cc[p])
        print('loop %.2f s, %d calls %.2f s' % (tl, len(pairs), tc), file=sys.stderr, flush=True)

    # ---- the scoring step alone
    rs = np.random.RandomState(0)
    logits = torch.from_numpy(rs.standard_normal((256, 1000)).astype(np.float32) * 4).cuda()
    labels = torch.from_numpy(rs.randint(0, 1000, 256)).cuda()
    labels[::3] = logits[::3].argmax(1)
    counters = torch.zeros(2, dtype=torch.int64, device='cuda')

    def hip():
        topk_score(logits, labels, ks=(1, 5), hits=counters, pred=False, rank=False)

    def hip_with_ranks():
        topk_score(logits, labels, ks=(1, 5), hits=counters)

    def torch_form():
        return S.topk_correct(logits, labels)

    hip()
    assert counters.tolist() == torch_form()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.reps

    for fn in (hip, hip_with_ranks, torch_form):
        window(fn)
    t = {'hip': [], 'hip_with_ranks': [], 'torch': []}
    for _ in range(a.windows):
        t['hip'].append(window(hip))
        t['hip_with_ranks'].append(window(hip_with_ranks))
        t['torch'].append(window(torch_form))

    def stat(v):
        return {'median': statistics.median(v), 'min': min(v), 'max': max(v)}
    out = {'device': torch.cuda.get_device_name(0), 'files': a.files, 'file_size': [375, 500], 'reader': 'hip', 'model': 'resnet50_official',
           'precision': 'bf16', 'batch_size': 256, 'pairs': len(pairs), 'rounds': a.rounds,
           'loop_seconds': stat(t_loop), 'loop_seconds_all': t_loop,
           'calls_seconds': stat(t_calls), 'calls_seconds_all': t_calls,
           'speedup_of_medians': statistics.median(t_calls) / statistics.median(t_loop),
           'pairs_whose_counts_differ': differing,
           'scoring_step': {'rows': 256, 'classes': 1000, 'reps': a.reps, 'windows': a.windows,
                            'what': 'host clock around back-to-back calls, a synchronise at the end of the window, microseconds per call',
                            'topk_score_counters_only_us': stat(t['hip']), 'topk_score_with_pred_and_rank_us': stat(t['hip_with_ranks']),
                            'topk_correct_us': stat(t['torch'])}}
    print(json.dumps(out))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
