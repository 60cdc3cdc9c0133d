"""The ImageNet-C and ImageNet-S evaluation loops of this tree against the parent commit's: the loops are host-paced, so the shared
scaffold of train/evaluate.py must not show up in their time.

    python profiles/solver_eval_refactor_ab.py --parent DIR [--files 256] [--alternations 3] [--out profiles/solver_eval_refactor_ab.json]

DIR holds the parent commit's tree with its library built.  The workload is that of profiles/imagenet_c_loop_ab.py: 256 JPEG files of
375 x 500 written from a seed, the 'hip' reader, ResNet-50 on the bf16 engine, one batch of 256, the torch module built once and
passed in.  A timed step is one whole evaluate() call -- `--imagenet-c` over 15 corruptions x 5 severities, or `--imagenet-s` over the
eleven operators -- between two synchronizes, engine construction included.  Each tree runs in a worker process of its own; after one
warm-up of each loop the driver asks parent and this tree in turn, --alternations times, and gives every step --step-timeout seconds:
a step that runs out, or a worker that ends, stops the job with nothing more started.  The returned metrics of the two trees are
compared as well.  Accepted: the median of this tree lies inside the parent's own min - max, or below it."""
import argparse
import contextlib
import io
import json
import os
import queue
import statistics
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(tree, root):
    sys.path[:0] = [tree, ROOT]
    import torch
    from profiles.imagenet_c_loop_ab import Args
    from robustart_amd.model import get_model
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    from robustart_amd.train import cls_solver as S
    assert os.path.realpath(S.__file__).startswith(os.path.realpath(tree) + os.sep), S.__file__
    cfg = {'model': {'type': 'resnet50_official'},
           'data': {'type': 'imagenet', 'read_from': 'fs', 'batch_size': 256, 'input_size': 224, 'test_resize': 256, 'num_workers': 8,
                    'test': {'root_dir': os.path.join(root, 'val'), 'meta_file': os.path.join(root, 'meta.txt'),
                             'image_reader': {'type': 'hip'}, 'transforms': {'type': 'ONECROP'},
                             'imagenet_c_frost_dir': os.path.join(root, 'frost')}}}
    torch.manual_seed(0)
    model = randomize_bn_stats(get_model(cfg['model'])).eval()
    rank, world, device = S.init_dist()
    print(json.dumps({'ready': True, 'device': torch.cuda.get_device_name(0)}), flush=True)
    for line in sys.stdin:
        if line.strip() not in ('imagenet_c', 'imagenet_s'):
            break
        x = Args()
        setattr(x, line.strip(), True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            res = S.evaluate(cfg, x, rank, world, device, model=model)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        res.pop('seconds')
        print(json.dumps({'s': t, 'result': res}), flush=True)


class Worker:
    def __init__(self, tree, root, step_timeout):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', tree, '--root', root],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        self.lines, self.step_timeout = queue.Queue(), step_timeout
        threading.Thread(target=self.read, daemon=True).start()
        self.device = self.ask(None)['device']

    def read(self):
        for line in self.p.stdout:
            self.lines.put(line)
        self.lines.put('')                                 # the worker's end

    def ask(self, cmd):
        if cmd is not None:
            self.p.stdin.write(cmd + '\n')
            self.p.stdin.flush()
        deadline = time.monotonic() + self.step_timeout
        while True:
            line = self.lines.get(timeout=max(deadline - time.monotonic(), 0.001))       # queue.Empty: the step ran out of time
            if not line:
                raise RuntimeError('worker ended (exit status %r) at %r' % (self.p.poll(), cmd))
            if line.startswith('{'):                       # anything else is a library's chatter
                return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None)
    ap.add_argument('--worker', default=None)
    ap.add_argument('--root', default=None)
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--alternations', type=int, default=3)
    ap.add_argument('--step-timeout', type=float, default=240.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.root)
    assert a.parent and os.path.isdir(a.parent), '--parent: the directory of the parent commit\'s tree'
    sys.path.insert(0, ROOT)
    from profiles.imagenet_c_loop_ab import write_files
    root = tempfile.mkdtemp()
    write_files(root, a.files)
    trees, loops = {}, ('imagenet_c', 'imagenet_s')
    try:
        for k, tree in (('parent', os.path.abspath(a.parent)), ('this', ROOT)):
            trees[k] = Worker(tree, root, a.step_timeout)
        times = {lp: {k: [] for k in trees} for lp in loops}
        same = True
        for alt in range(a.alternations + 1):              # round 0 is the warm-up of each loop in each tree
            for lp in loops:
                got = {k: w.ask(lp) for k, w in trees.items()}                           # parent, then this tree
                same = same and got['parent']['result'] == got['this']['result']
                for k in trees:
                    if alt:
                        times[lp][k].append(got[k]['s'])
                print('%s round %d: parent %.4f s, this %.4f s' % (lp, alt, got['parent']['s'], got['this']['s']), file=sys.stderr, flush=True)
        for w in trees.values():
            w.p.stdin.close()
            w.p.wait(timeout=60)
    finally:
        for w in trees.values():                           # after a time-out or a worker's end: nothing more runs
            if w.p.poll() is None:
                w.p.kill()
    res = {'device': trees['this'].device, 'files': a.files, 'file_size': [375, 500], 'reader': 'hip', 'model': 'resnet50_official',
           'precision': 'bf16', 'batch_size': 256, 'alternations': a.alternations, 'cpus_available': len(os.sched_getaffinity(0)),
           'what': 'seconds of one evaluate() call between two synchronizes, parent and this tree in turn in one job',
           'results_identical': same}
    for lp in loops:
        p, t = times[lp]['parent'], times[lp]['this']
        res[lp + '_loop_seconds'] = {'parent': {'median': statistics.median(p), 'min': min(p), 'max': max(p), 'all': p},
                                     'this': {'median': statistics.median(t), 'min': min(t), 'max': max(t), 'all': t},
                                     'this_median_within_parents_range_or_below': statistics.median(t) <= max(p)}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
