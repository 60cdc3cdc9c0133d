"""ResNeXt's grouped 3x3 (csrc/conv_grouped.hip) against the same convolution through the generic entries, and the whole network.
Every figure of profiles/grouped_conv_ab.json comes from one of these modes; each writes its own section of the file (--out):

    python profiles/grouped_conv_ab.py shapes --out FILE [--batch 256]
        every conv2 shape of resnext50_32x4d at 224 x 224 (layer1 stride 1; layers 2-4 stride 2 and stride 1), forward (bias + ReLU + sign
        tensor) and backward (1-bit mask; the four classes at stride 2), both precisions: `grouped_conv_kernel` on / off alternating, one
        process, ten warm-up launches per side, seven groups of twenty launches per side; medians with min-max, and the achieved bytes / time
        of the new kernel against the launch's algorithmic bytes (source + destination + masks once)
    python profiles/grouped_conv_ab.py grad --out FILE [--batch 256]
        one gradient evaluation of resnext50_32x4d, switch on / off alternating, both precisions; ResNet-50's figure beside it for scale
    python profiles/grouped_conv_ab.py bench --parent DIR --out FILE [--rounds 3]
        bench.py --gpus 1 --steps 20 --warmup 5 (ResNet-50), the parent tree (library built) and this tree alternating in child processes

Operands are random: a convolution's time does not depend on their values."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _section(out_path, name, value):
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc[name] = value
    json.dump(doc, open(out_path, 'w'), indent=1)


def _stats(v):
    return {'median': round(statistics.median(v), 1), 'min': round(min(v), 1), 'max': round(max(v), 1)}


def _time(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us


def shapes(out_path, batch):
    import torch
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import ResNet50Engine
    torch.manual_seed(0)
    model = get_model({'type': 'resnext50_32x4d'}).eval()
    res = {}
    what = ('us per convolution at B = %d (10 warm-up launches per side, then groups of 20 launches, 7 groups per side, sides alternating, one '
            'process); generic = rart_conv_igemm_bf16 / rart_gemm_pair_bf16, one launch per slice (and class)' % batch)
    for precision in ('bf16', 'fp32x'):
        eng = ResNet50Engine(model, 'cuda', precision)
        x3 = eng.x3
        lead = (2, batch) if x3 else (batch,)
        seen, hw = set(), (56, 56)
        for ca, cb, cc, ds in eng.blocks:
            xhw, ohw = hw, (hw[0] // cb.stride, hw[1] // cb.stride)
            hw = ohw
            key = (cb.cin, cb.gw, cb.stride, xhw)
            if key in seen:
                continue
            seen.add(key)
            C = cb.cin
            g = torch.Generator(device='cuda').manual_seed(C)
            rnd = lambda *s: torch.randn(*s, generator=g, device='cuda').to(torch.bfloat16)        # noqa: E731
            bits = lambda h: torch.randint(0, 256, (batch, h[0], h[1], C // 8), generator=g, device='cuda', dtype=torch.uint8)  # noqa: E731
            x, y, dx = rnd(*lead, xhw[0], xhw[1], C), rnd(*lead, ohw[0], ohw[1], C), torch.empty(*lead, xhw[0], xhw[1], C, dtype=torch.bfloat16, device='cuda')
            sign, mask = bits(ohw), bits(xhw)
            runs = {'fwd': lambda: eng._conv_fwd(cb, x, xhw, y, True, sign=sign, pair=x3),
                    'bwd': lambda: eng._conv_bwd(cb, y, ohw, dx, xhw, mask=mask, pair=x3)}
            eb = 4.0 if x3 else 2.0
            px_in, px_out = batch * xhw[0] * xhw[1], batch * ohw[0] * ohw[1]
            nbytes = {'fwd': eb * C * (px_in + px_out) + px_out * C / 8.0, 'bwd': eb * C * (px_in + px_out) + px_in * C / 8.0}
            for direction, fn in runs.items():
                reps = 20
                us = {True: [], False: []}
                for on in (True, False):
                    eng.grouped_conv_kernel = on
                    _time(fn, 10)
                for _ in range(7):
                    for on in (True, False):
                        eng.grouped_conv_kernel = on
                        us[on].append(_time(fn, reps))
                eng.grouped_conv_kernel = True
                new, old = _stats(us[True]), _stats(us[False])
                name = '%s C%d gw%d stride%d %dx%d %s' % (precision, C, cb.gw, cb.stride, xhw[0], xhw[1], direction)
                res[name] = {'us_new_kernel': new, 'us_generic_entries': old, 'speedup_of_medians': round(old['median'] / new['median'], 2),
                             'new_kernel_wins_beyond_spread': bool(new['max'] < old['min']),
                             'algorithmic_MB': round(nbytes[direction] / 1e6, 1),
                             'new_kernel_TB_per_s': round(nbytes[direction] / new['median'] / 1e6, 2),
                             'generic_launches': (C // cb.slice) * (1 if (direction == 'fwd' or cb.stride == 1) else 4)}
                print(name, res[name], flush=True)
                _section(out_path, 'shapes', {'what': what, 'results': res})
            del x, y, dx, sign, mask
        del eng
        torch.cuda.empty_cache()


def _grad_ms(eng, batch, rounds, switch):
    """ms per gradient evaluation (three back to back); switch: alternate `grouped_conv_kernel` on / off, else one side"""
    import torch
    x = torch.rand(batch, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (batch,), device='cuda')
    sides = (True, False) if switch else (True,)
    ms = {s: [] for s in sides}
    for r in range(rounds + 1):
        for on in sides:
            eng.grouped_conv_kernel = on
            t = _time(lambda: eng.forward_backward(x, MEAN, STD, y, 0), 3) / 1e3
            if r:                           # round 0 warms both sides up
                ms[on].append(t)
    eng.grouped_conv_kernel = True
    return {('new_kernel' if s else 'generic_entries'): {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
            for s, v in ms.items()}


def grad(out_path, batch):
    import torch
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import ResNet50Engine
    res = {}
    for precision in ('bf16', 'fp32x'):
        torch.manual_seed(0)
        eng = ResNet50Engine(get_model({'type': 'resnext50_32x4d'}).eval(), 'cuda', precision)
        res['resnext50_32x4d ' + precision] = _grad_ms(eng, batch, 4, True)
        del eng
        torch.cuda.empty_cache()
        eng = ResNet50Engine(get_model({'type': 'resnet50_official'}).eval(), 'cuda', precision)
        res['resnet50_official ' + precision] = _grad_ms(eng, batch, 4, False)['new_kernel']
        del eng
        torch.cuda.empty_cache()
        print(precision, {k: v for k, v in res.items() if k.endswith(precision)}, flush=True)
    _section(out_path, 'gradient_evaluation', {'what': 'forward_backward at B = %d, 224 x 224, ms per evaluation (three back to back, four groups per side, '
                                                       'sides alternating after a warm-up round)' % batch, 'results': res})


def bench(parent, out_path, rounds):
    trees = [('parent', os.path.abspath(parent)), ('tree', HERE)]
    runs = {k: [] for k, _ in trees}
    for r in range(rounds):
        for name, root in trees:
            p = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '20', '--warmup', '5'], cwd=root, capture_output=True,
                               text=True, timeout=280)
            if p.returncode != 0:                      # a child that failed ends the job: nothing more is started on the GPU
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit('bench failed in %s (round %d, exit %d)' % (name, r, p.returncode))
            j = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
            runs[name].append(j['ms_per_step'])
            print(name, r, round(j['ms_per_step'], 3), flush=True)
    _section(out_path, 'bench_resnet50', {'command': 'python bench.py --gpus 1 --steps 20 --warmup 5, the parent commit and this tree alternating in child '
                                                     'processes, %d runs per side' % rounds, 'ms_per_step': runs,
                                          'median_ms_per_step': {k: statistics.median(v) for k, v in runs.items()},
                                          'spread_max_minus_min_ms': {k: max(v) - min(v) for k, v in runs.items()}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['shapes', 'grad', 'bench'])
    ap.add_argument('--out', required=True)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--parent')
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    if a.mode == 'shapes':
        return shapes(a.out, a.batch)
    if a.mode == 'grad':
        return grad(a.out, a.batch)
    return bench(a.parent, a.out, a.rounds)


if __name__ == '__main__':
    main()
