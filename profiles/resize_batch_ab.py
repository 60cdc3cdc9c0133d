"""FileImageNet.batch with the batched variable-size resize against the parent commit's per-image resize loop, and the ImageNet-S
loop's time split -- the numbers of DESIGN.md 4.5.4 / 4.9.

    python profiles/resize_batch_ab.py --parent DIR [--images 256] [--reps 5] [--out profiles/resize_batch_ab.json]

DIR holds the parent commit's tree with its library built (`git archive HEAD^ | tar -x -C DIR`, then DIR/robustart_amd/csrc/build.py).
The workload is the 256 files of 375 x 500 of profiles/jpeg_reader_ab.py; the variants are batch() under ONECROP and STANDARD with the
readers 'pil' and 'hip' (8 workers).  Each tree runs in a worker process of its own (both packages have one name); the driver asks the
two workers for one timed batch() in turn, so parent and this tree alternate inside every repetition on one box.  The outputs are
compared first, bit for bit (sha256 of the batch's bytes).  Wall clock with a synchronize inside, median of --reps after a warm-up
round, with the min - max of both.  Also: the resize share alone (this tree: the time around the transform step; the parent has no
such step, so its share is batch() minus its decode step timed alone), and the ImageNet-S loop on this tree for 256 images, split
into decode / eleven resizes / eleven forwards (ResNet-50, bf16 engine, random weights)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(t, r) for t in ('ONECROP', 'STANDARD') for r in ('pil', 'hip')]
NUM_WORKERS = 8


def worker(tree, folder, images):
    """one tree's side: answers 'batch T R', 'decode T R', 'transform T R' and 'loop' with one JSON line each"""
    sys.path.insert(0, tree)
    import torch
    from robustart_amd.train import cls_solver as S
    assert os.path.realpath(S.__file__).startswith(os.path.realpath(tree)), S.__file__
    dev = torch.device('cuda')
    sets = {(t, r): S.FileImageNet.from_folder(folder, 224, 256, t, reader=r, seed=1, num_workers=NUM_WORKERS) for t, r in VARIANTS}
    idx = list(range(images))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def decode(ds):
        if hasattr(ds, 'decode_indices'):
            return ds.decode_indices(idx, dev)
        if ds.reader == 'hip':
            return ds.decode_batch(idx, dev)
        return [torch.from_numpy(ds.decode(i)[0]).to(dev, non_blocking=True) for i in idx]

    print(json.dumps({'ready': True}), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == 'quit':
            break
        if cmd[0] == 'loop':
            print(json.dumps(loop(S, sets[('ONECROP', 'hip')], idx, dev, timed)), flush=True)
            continue
        ds = sets[(cmd[1], cmd[2])]
        if cmd[0] == 'batch':
            t, (out, _) = timed(lambda: ds.batch(idx, dev))
            res = {'s': t, 'sha256': hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()}
        elif cmd[0] == 'decode':
            res = {'s': timed(lambda: decode(ds))[0]}
        else:                                              # 'transform': this tree only
            decoded = decode(ds)
            res = {'s': timed(lambda: ds.transform_batch(decoded, idx, 0))[0]}
        print(json.dumps(res), flush=True)


def loop(S, ds, idx, dev, timed):
    """the ImageNet-S loop's three parts on one decoded batch, each timed with a synchronize; second pass of two (the first warms up)"""
    import torch
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import EngineModel
    from robustart_amd.noise import imagenet_s as NS
    torch.manual_seed(0)
    eng = EngineModel(get_model({'type': 'resnet50_official'}).to(dev).eval(), takes_normalized=False, precision='bf16').rart_engine
    ops = S.imagenet_s_ops(None)
    for rep in range(2):
        res = {'decode_ms': 0.0, 'resize_ms': {}, 'forward_ms': {}}
        t, decoded = timed(lambda: ds.decode_indices(idx, dev))
        res['decode_ms'] = 1e3 * t
        for op in ops:
            t, imgs = timed(lambda: NS.image_transfer_batch(None, 'pil', op, 'val', 224, ds.num_workers, decoded=decoded))
            res['resize_ms'][op] = 1e3 * t
            res['forward_ms'][op] = 1e3 * timed(lambda: eng.logits_from_u8(imgs, S.IMAGENET_MEAN, S.IMAGENET_STD))[0]
    res['resize_pil_ms'] = sum(v for k, v in res['resize_ms'].items() if k.startswith('pil-'))
    res['resize_opencv_ms'] = sum(v for k, v in res['resize_ms'].items() if k.startswith('opencv-'))
    res['forward_total_ms'] = sum(res['forward_ms'].values())
    total = res['decode_ms'] + res['resize_pil_ms'] + res['resize_opencv_ms'] + res['forward_total_ms']
    res['total_ms'], res['opencv_share'] = total, res['resize_opencv_ms'] / total
    return res


class Worker:
    def __init__(self, tree, folder, images):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', tree, '--folder', folder, '--images', str(images)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert self.ask(None)['ready']

    def ask(self, cmd):
        if cmd is not None:
            self.p.stdin.write(cmd + '\n')
            self.p.stdin.flush()
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError('worker ended (exit status %r) at %r' % (self.p.poll(), cmd))
            if line.startswith('{'):                       # anything else is a library's chatter
                return json.loads(line)

    def close(self):
        self.p.stdin.write('quit\n')
        self.p.stdin.close()
        self.p.wait(timeout=60)


def stats(ts):
    return {'median_ms': 1e3 * statistics.median(ts), 'min_ms': 1e3 * min(ts), 'max_ms': 1e3 * max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None)
    ap.add_argument('--worker', default=None)
    ap.add_argument('--folder', default=None)
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.folder, a.images)
    assert a.parent and os.path.isdir(a.parent), '--parent: the directory of the parent commit\'s tree'
    sys.path.insert(0, ROOT)
    from profiles.jpeg_reader_ab import write_files
    with tempfile.TemporaryDirectory() as folder:
        write_files(folder, a.images)
        trees = {'parent': Worker(os.path.abspath(a.parent), folder, a.images), 'this': Worker(ROOT, folder, a.images)}
        try:
            res = {'images': a.images, 'image_hw': [375, 500], 'reps': a.reps, 'num_workers': NUM_WORKERS,
                   'cpus_available': len(os.sched_getaffinity(0)), 'variants': {}}
            times = {(v, k): [] for v in VARIANTS for k in trees}
            for rep in range(a.reps + 1):                  # round 0 is the warm-up; it also compares the outputs
                for v in VARIANTS:
                    got = {k: w.ask('batch %s %s' % v) for k, w in trees.items()}      # parent, then this tree
                    assert got['parent']['sha256'] == got['this']['sha256'], ('outputs differ', v, rep)
                    if rep:
                        for k in trees:
                            times[(v, k)].append(got[k]['s'])
            for v in VARIANTS:
                p, t = stats(times[(v, 'parent')]), stats(times[(v, 'this')])
                dec = stats([trees['parent'].ask('decode %s %s' % v)['s'] for _ in range(a.reps + 1)][1:])
                tr = stats([trees['this'].ask('transform %s %s' % v)['s'] for _ in range(a.reps + 1)][1:])
                res['variants']['%s/%s' % v] = {
                    'parent': p, 'this': t, 'outputs_identical': True, 'speedup': p['median_ms'] / t['median_ms'],
                    'this_slower_beyond_parents_range': t['median_ms'] > p['max_ms'],
                    'parent_decode_alone': dec, 'parent_resize_share_ms': p['median_ms'] - dec['median_ms'], 'this_transform_step': tr}
            res['imagenet_s_loop'] = trees['this'].ask('loop')
        finally:
            for w in trees.values():
                w.close()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
