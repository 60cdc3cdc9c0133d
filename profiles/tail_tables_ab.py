"""Headline step with the layer1 tail kernel's expansion table staged in LDS, against a checkout of the parent commit (library built):
`python bench.py --gpus 1 --steps 20 --warmup 5` in fresh child processes, the two trees alternating, ROUNDS runs per side; round 0 with
--dump-outputs on both sides, every array compared with numpy.array_equal.  Writes the JSON that profiles/tail_tables_ab.json keeps.

    python profiles/tail_tables_ab.py --parent DIR --out FILE [--rounds 4]"""
import argparse, json, os, statistics, subprocess, sys, tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--parent', required=True)
ap.add_argument('--out', required=True)
ap.add_argument('--rounds', type=int, default=4)
a = ap.parse_args()
trees = [('parent', os.path.abspath(a.parent)), ('lds', HERE)]
tmp = tempfile.mkdtemp()
runs = {k: [] for k, _ in trees}
for r in range(a.rounds):
    for name, root in trees:
        cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '20', '--warmup', '5']
        if r == 0:
            cmd += ['--dump-outputs', os.path.join(tmp, name)]
        p = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=280)
        if p.returncode != 0:                      # a child that failed ends the job: nothing more is started on the GPU
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit('bench failed in %s (round %d, exit %d)' % (name, r, p.returncode))
        j = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
        runs[name].append(j['ms_per_step'])
        print(name, r, round(j['ms_per_step'], 3), j['dtype'], flush=True)
med = {k: statistics.median(v) for k, v in runs.items()}
spread = {k: max(v) - min(v) for k, v in runs.items()}
gain = med['parent'] - med['lds']
bar = 3 * max(spread.values())
outs = {}
for f in sorted(os.listdir(os.path.join(tmp, 'parent'))):
    x, y = np.load(os.path.join(tmp, 'parent', f)), np.load(os.path.join(tmp, 'lds', f))
    outs[f] = {'array_equal': bool(np.array_equal(x, y))}
res = {'what': 'headline bench, reference precision, B = 256, one MI355X: the parent commit against the layer1 tail kernel with the '
               'expansion table staged in LDS once per workgroup',
       'command': 'python bench.py --gpus 1 --steps 20 --warmup 5 (one job, the two trees alternating in child processes, %d runs per side, '
                  'profiler off); round 0 with --dump-outputs DIR on both sides' % a.rounds,
       'ms_per_step': runs, 'median_ms_per_step': med, 'spread_max_minus_min_ms': spread, 'gain_ms_per_step': gain,
       'gain_percent': 100 * gain / med['parent'], 'bar_ms': bar, 'every_lds_run_below_every_parent_run': max(runs['lds']) < min(runs['parent']),
       'clears_the_bar': bool(max(runs['lds']) < min(runs['parent']) and gain >= bar), 'outputs': outs}
json.dump(res, open(a.out, 'w'), indent=1)
print(json.dumps({k: res[k] for k in ('median_ms_per_step', 'spread_max_minus_min_ms', 'gain_ms_per_step', 'bar_ms', 'clears_the_bar')}))
print('outputs array_equal:', all(v['array_equal'] for v in outs.values()), len(outs))
