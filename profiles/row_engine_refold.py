"""Host time of `refold()` on the GPU for ViT-B/16 and ConvNeXt-B in both precisions (the shared launch layer): wall clock
around one refold that ends in a device synchronise, median / min / max of N calls after warm-up.

    python profiles/row_engine_refold.py [--calls 30] [--warmup 5] [--tree DIR] [--out result.json]
    python profiles/row_engine_refold.py --ab PARENT_DIR [--out profiles/row_engine_host_ab.json]

`refold` rebuilds every weight table from the module's parameters and runs once per iteration of adversarial training; it is torch
ops and allocations on the host's account, no kernel of the library.  --tree names the checkout whose package is timed (default: the
one this file lies in).  --ab compares that checkout with a built checkout of another commit in one session, alternating the two,
one fresh process per measurement: this script twice per tree, then `bench.py --workload vit_pgd` and `--workload vit_inc` three
times per tree.  It writes every figure, and per figure whether this tree's median lies inside the other tree's min-max."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('vit_base/bf16', 'vit_base/fp32x', 'convnext_base/bf16', 'convnext_base/fp32x')


def child(cmd, cwd, limit=300):
    """-> the JSON object on the last output line of one measurement process; a failure ends the session"""
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.exit('%s in %s ended with status %d:\n%s' % (' '.join(cmd), cwd, r.returncode, r.stderr[-2000:]))
    return json.loads([line for line in r.stdout.splitlines() if line.startswith('{')][-1])


def spread(vals):
    return {'median': statistics.median(vals), 'min': min(vals), 'max': max(vals), 'runs': vals}


def ab(a):
    trees = (('parent', os.path.abspath(a.ab)), ('this', a.tree))
    refold = {t: {c: [] for c in CASES} for t, _ in trees}
    bench = {t: {w: [] for w in ('vit_pgd', 'vit_inc')} for t, _ in trees}
    for i in range(2):
        for t, d in trees:
            r = child([sys.executable, os.path.abspath(__file__), '--tree', d, '--calls', str(a.calls), '--warmup', str(a.warmup)], d)
            for c in CASES:
                refold[t][c].append(r[c])
            print('refold', t, i, {c: round(r[c]['median'], 2) for c in CASES}, flush=True)
    for w in bench['this']:
        for i in range(3):
            for t, d in trees:
                r = child([sys.executable, 'bench.py', '--gpus', '1', '--steps', '10', '--warmup', '3', '--workload', w], d)
                bench[t][w].append(r['ms_per_step'])
                print('bench', w, t, i, round(r['ms_per_step'], 2), flush=True)
    res = {'unit': 'ms', 'refold_calls_per_run': a.calls, 'bench': '--gpus 1 --steps 10 --warmup 3, ms_per_step',
           'refold': {}, 'bench_ms_per_step': {}, 'inside_parent_min_max': {}}
    for c in CASES:      # per tree: the median of the runs' medians, the extremes over every call of every run
        res['refold'][c] = {t: {'median': statistics.median(r['median'] for r in refold[t][c]), 'min': min(r['min'] for r in refold[t][c]),
                                'max': max(r['max'] for r in refold[t][c]), 'run_medians': [r['median'] for r in refold[t][c]]}
                            for t, _ in trees}
    for w in bench['this']:
        res['bench_ms_per_step'][w] = {t: spread(bench[t][w]) for t, _ in trees}
    for k, v in list(res['refold'].items()) + list(res['bench_ms_per_step'].items()):
        res['inside_parent_min_max'][k] = v['parent']['min'] <= v['this']['median'] <= v['parent']['max']
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--ab', metavar='PARENT_DIR', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.tree = os.path.abspath(a.tree)
    if a.ab:
        return ab(a)
    sys.path.insert(0, a.tree)
    import torch
    from robustart_amd.model import get_model
    from robustart_amd.model.convnext_engine import ConvNeXtEngine
    from robustart_amd.model.vit_engine import ViTEngine
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    res = {'calls': a.calls, 'warmup': a.warmup, 'unit': 'ms'}
    for name, cfg, cls in (('vit_base', {'type': 'vit_base'}, ViTEngine), ('convnext_base', {'type': 'convnext_base'}, ConvNeXtEngine)):
        torch.manual_seed(0)
        model = get_model(cfg).cuda().eval()
        for precision in ('bf16', 'fp32x'):
            eng = cls(model, 'cuda', precision)
            ms = []
            for i in range(a.warmup + a.calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.refold(model)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            ms = ms[a.warmup:]
            res['%s/%s' % (name, precision)] = {'median': statistics.median(ms), 'min': min(ms), 'max': max(ms)}
            del eng
        del model
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
