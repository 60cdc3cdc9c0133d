"""DenseNet-121 on DenseNetEngine at B = 256, 224 x 224: what the new kernels of csrc/densenet.hip cost per launch, and the whole network.
Every figure of profiles/densenet_preact_ab.json comes from one of these modes; each writes its own section of the file (--out):

    python profiles/densenet_preact_ab.py launches --out FILE [--batch 256]
        one gradient evaluation with the engine's launch profile on, after two warm-up evaluations, three times; per launch kind the
        count, the summed time and the summed algorithmic bytes; per distinct launch of the new kernels (kind, channels, rows) the
        median time over the three evaluations, its algorithmic bytes and the achieved bytes / time
    python profiles/densenet_preact_ab.py grad --out FILE [--batch 256]
        forward (logits) and gradient evaluation (forward_backward) in ms, both precisions, ResNet-50 beside it for scale, and a
        PGD-3 evaluation (pgd_linf, eps 4/255, through EngineModel) in images / s

Inputs are random: no launch's time depends on the values."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _section(out_path, name, value):
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc[name] = value
    json.dump(doc, open(out_path, 'w'), indent=1)


def _time(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps          # ms


def _stats(v, nd=3):
    return {'median': round(statistics.median(v), nd), 'min': round(min(v), nd), 'max': round(max(v), nd)}


def launches(out_path, batch):
    import torch
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import make_engine
    res = {}
    for precision in ('bf16', 'fp32x'):
        torch.manual_seed(0)
        eng = make_engine(get_model({'type': 'densenet121'}).eval(), 'cuda', precision)
        x = torch.rand(batch, 3, 224, 224, device='cuda')
        y = torch.randint(0, 1000, (batch,), device='cuda')
        for _ in range(2):
            eng.forward_backward(x, MEAN, STD, y, 0)
        runs = []
        for _ in range(3):
            eng.profile = []
            eng.forward_backward(x, MEAN, STD, y, 0)
            torch.cuda.synchronize()
            runs.append([(r[3], r[1].elapsed_time(r[2]) * 1e3, r[4] if len(r) > 4 and r[4] else 0.0, r[0]) for r in eng.profile])
            eng.profile = None
        kinds = {}
        for i, (kind, _, nbytes, flops) in enumerate(runs[0]):
            us = statistics.median(r[i][1] for r in runs)
            k = kinds.setdefault(kind, {'launches': 0, 'us': 0.0, 'algorithmic_MB': 0.0, 'GFLOP': 0.0})
            k['launches'] += 1
            k['us'] += us
            k['algorithmic_MB'] += nbytes / 1e6
            k['GFLOP'] += flops / 1e9
        for k in kinds.values():
            k.update(us=round(k['us'], 1), algorithmic_MB=round(k['algorithmic_MB'], 1), GFLOP=round(k['GFLOP'], 1))
            if k['algorithmic_MB']:
                k['TB_per_s'] = round(k['algorithmic_MB'] / k['us'], 2)
        per = {}
        for i, (kind, _, nbytes, _) in enumerate(runs[0]):
            if kind.startswith('dn_'):
                per.setdefault((kind, nbytes), []).append(statistics.median(r[i][1] for r in runs))
        rows = [{'kind': kind, 'algorithmic_MB': round(nbytes / 1e6, 1), 'launches': len(v), 'us_median': round(statistics.median(v), 1),
                 'TB_per_s': round(nbytes / 1e6 / statistics.median(v), 2), 'of_8_TB_per_s': round(nbytes / 1e6 / statistics.median(v) / 8.0, 2)}
                for (kind, nbytes), v in sorted(per.items(), key=lambda kv: (kv[0][0], kv[0][1]))]
        res[precision] = {'by_kind': kinds, 'total_us': round(sum(k['us'] for k in kinds.values()), 1), 'new_kernels_by_launch': rows}
        print(precision, json.dumps(res[precision]['by_kind']), flush=True)
        _section(out_path, 'launches', {'what': 'densenet121, one gradient evaluation at B = %d with the launch profile on (events around every launch, so '
                                                'the sum exceeds the unprofiled evaluation); medians over three evaluations after two warm-up ones; '
                                                'algorithmic bytes = every operand once' % batch, 'results': res})
        del eng
        torch.cuda.empty_cache()


def grad(out_path, batch):
    import torch
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import EngineModel, make_engine
    from robustart_amd.noise import AddNoise
    res = {}
    for precision in ('bf16', 'fp32x'):
        for mtype in ('densenet121', 'resnet50_official'):
            torch.manual_seed(0)
            model = get_model({'type': mtype}).eval()
            eng = make_engine(model, 'cuda', precision)
            x = torch.rand(batch, 3, 224, 224, device='cuda')
            y = torch.randint(0, 1000, (batch,), device='cuda')
            fwd, bwd = [], []
            for r in range(5):
                a, b = _time(lambda: eng.logits(x, MEAN, STD), 3), _time(lambda: eng.forward_backward(x, MEAN, STD, y, 0), 3)
                if r:                           # round 0 warms up
                    fwd.append(a)
                    bwd.append(b)
            entry = {'forward_ms': _stats(fwd), 'gradient_evaluation_ms': _stats(bwd),
                     'gradient_evaluations_images_per_s': round(batch / statistics.median(bwd) * 1e3)}
            if mtype == 'densenet121':
                f = EngineModel(model, takes_normalized=False, engine=eng)
                att = AddNoise('pgd_linf')
                att.set_config(f_model=f, eps=4 / 255, steps=3)
                pgd = []
                for r in range(4):
                    t = _time(lambda: att.add_noise(x, y), 1)
                    if r:
                        pgd.append(t)
                entry['pgd3_ms_per_batch'] = _stats(pgd)
                entry['pgd3_images_per_s'] = round(batch / statistics.median(pgd) * 1e3)
            res['%s %s' % (mtype, precision)] = entry
            print(mtype, precision, entry, flush=True)
            _section(out_path, 'network', {'what': 'B = %d, 224 x 224; ms per call (three back to back, four groups after a warm-up group); pgd3 = '
                                                   'AddNoise(pgd_linf, eps 4/255, 3 steps) through EngineModel, one batch per call, three calls '
                                                   'after a warm-up call' % batch, 'results': res})
            del eng
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['launches', 'grad'])
    ap.add_argument('--out', required=True)
    ap.add_argument('--batch', type=int, default=256)
    a = ap.parse_args()
    return launches(a.out, a.batch) if a.mode == 'launches' else grad(a.out, a.batch)


if __name__ == '__main__':
    main()
