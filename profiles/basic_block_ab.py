"""The fused BasicBlock kernel (csrc/basic_block.hip) against the conv-by-conv route of the same tree, and the whole networks.
Every figure of profiles/basic_block_ab.json comes from one of these modes; each writes its own section of the file (--out):

    python profiles/basic_block_ab.py shapes --out FILE [--batch 256]
        the identity blocks of layer1 (64 @ 56 x 56) and layer2 (128 @ 28 x 28), forward (biases + ReLU + both sign tensors) and backward
        (both 1-bit masks): one rart_basic_block_bf16 launch against the two launches of the conv-by-conv route, alternating, one process,
        ten warm-up launches per side, seven groups of twenty launches per side; medians with min-max, the algorithmic MB (x + out + the
        1-bit tensors once) and the fused launch's TB/s against them
    python profiles/basic_block_ab.py grad --out FILE [--batch 256]
        one gradient evaluation of resnet18_official and resnet34_official: bf16 with `basic_block_kernel` on / off alternating, 'fp32x',
        and resnet50_official by the same loop for scale
    python profiles/basic_block_ab.py bench --parent DIR --out FILE [--rounds 3]
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


def _stats(v, nd=1):
    return {'median': round(statistics.median(v), nd), 'min': round(min(v), nd), 'max': round(max(v), nd)}


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
    from robustart_amd.model.basic_resnet_engine import BasicResNetEngine
    torch.manual_seed(0)
    eng = BasicResNetEngine(get_model({'type': 'resnet18_official'}).eval(), 'cuda', 'bf16')
    what = ('us per identity BasicBlock at B = %d (10 warm-up launches per side, then groups of 20, 7 groups per side, sides alternating, one '
            'process); fused = one rart_basic_block_bf16 launch, conv by conv = its two launches' % batch)
    res, hw, seen = {}, (56, 56), set()
    for c1, c2, ds in eng.basic:
        xhw, hw = hw, (hw[0] // c1.stride, hw[1] // c1.stride)
        if ds is not None or c1.cin in seen or not eng.lib.rart_basic_block_supported(c1.cin, xhw[0], xhw[1]):
            continue
        seen.add(c1.cin)
        C, B = c1.cin, batch
        g = torch.Generator(device='cuda').manual_seed(C)
        rnd = lambda: torch.randn(B, xhw[0], xhw[1], C, generator=g, device='cuda').to(torch.bfloat16)                        # noqa: E731
        bits = lambda: torch.randint(0, 256, (B, xhw[0], xhw[1], C // 8), generator=g, device='cuda', dtype=torch.uint8)      # noqa: E731
        x, mid, y = rnd(), rnd(), rnd()
        sa, so = bits(), bits()

        def fwd_fused():
            eng._basic(x, c1.w_fwd_frag, c2.w_fwd_frag, c1.bias, c2.bias, sa, so, y, B, xhw, C, c1.fwd_taps, False)

        def fwd_convs():
            eng._conv_fwd(c1, x, xhw, mid, True, sign=sa)
            eng._conv_fwd(c2, mid, xhw, y, True, res=x, sign=so)

        def bwd_fused():
            eng._basic(x, c2.w_bwd_frag, c1.w_bwd_frag, None, None, sa, so, y, B, xhw, C, c2.bwd[0][1], True)

        def bwd_convs():
            eng._conv_bwd(c2, x, xhw, mid, xhw, mask=sa)
            eng._conv_bwd(c1, mid, xhw, y, xhw, res=x, mask=so)
        nbytes = 2.0 * 2 * B * xhw[0] * xhw[1] * C + 2 * B * xhw[0] * xhw[1] * C / 8.0
        for direction, sides in (('fwd', (fwd_fused, fwd_convs)), ('bwd', (bwd_fused, bwd_convs))):
            us = ([], [])
            for fn in sides:
                _time(fn, 10)
            for _ in range(7):
                for i, fn in enumerate(sides):
                    us[i].append(_time(fn, 20))
            new, old = _stats(us[0]), _stats(us[1])
            name = 'bf16 C%d %dx%d %s' % (C, xhw[0], xhw[1], direction)
            res[name] = {'us_fused': new, 'us_conv_by_conv': old, 'speedup_of_medians': round(old['median'] / new['median'], 2),
                         'fused_slowest_group_below_conv_by_conv_fastest': bool(new['max'] < old['min']),
                         'algorithmic_MB': round(nbytes / 1e6, 1), 'fused_TB_per_s': round(nbytes / new['median'] / 1e6, 2),
                         'conv_by_conv_TB_per_s_on_the_same_bytes': round(nbytes / old['median'] / 1e6, 2)}
            print(name, res[name], flush=True)
            _section(out_path, 'shapes', {'what': what, 'results': res})
        del x, mid, y, sa, so
    torch.cuda.empty_cache()


def _grad_ms(eng, batch, rounds, switch):
    """ms per gradient evaluation (three back to back); switch: alternate `basic_block_kernel` on / off, else one side"""
    import torch
    x = torch.rand(batch, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (batch,), device='cuda')
    sides = (True, False) if switch else (True,)
    if switch:                              # the fused side takes every width the kernel serves, whatever the default list says
        from robustart_amd.model.basic_resnet_engine import BASIC_BLOCK_SERVED
        eng.basic_block_widths = BASIC_BLOCK_SERVED
    ms = {s: [] for s in sides}
    for r in range(rounds + 1):
        for on in sides:
            eng.basic_block_kernel = on
            t = _time(lambda: eng.forward_backward(x, MEAN, STD, y, 0), 3) / 1e3
            if r:                           # round 0 warms both sides up
                ms[on].append(t)
    eng.basic_block_kernel = True
    return {('fused' if s else 'conv_by_conv'): _stats(v, 3) for s, v in ms.items()}


def grad(out_path, batch):
    import torch
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import make_engine
    res = {}
    for mtype in ('resnet18_official', 'resnet34_official', 'resnet50_official'):
        for precision in ('bf16', 'fp32x'):
            torch.manual_seed(0)
            eng = make_engine(get_model({'type': mtype}).eval(), 'cuda', precision)
            both = precision == 'bf16' and mtype != 'resnet50_official'
            r = _grad_ms(eng, batch, 4, both)
            res['%s %s' % (mtype, precision)] = r if both else r['fused']
            print(mtype, precision, res['%s %s' % (mtype, precision)], flush=True)
            del eng
            torch.cuda.empty_cache()
            _section(out_path, 'gradient_evaluation', {'what': 'forward_backward at B = %d, 224 x 224, ms per evaluation (three back to back, four '
                                                               'groups per side, sides alternating after a warm-up round); bf16 ResNet-18 / -34 with '
                                                               '`basic_block_kernel` on (fused) and off (conv_by_conv)' % batch, 'results': res})


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
