"""The pair epilogue (gp_epilogue, csrc/rart_gemm_pair_dev.h) against the parent commit's library.  Every figure of
profiles/pair_epilogue_ab.json comes from one of these modes; --key names the entry a run writes.  The entries `wait_only`, `three_way`
and `whole_step_wait_only` were measured on LAB libraries (the counted wait alone, with and without the same wait in the tail kernel's
chunk loop; the wait + a second operand set) whose sources are not kept: the tree has no switch that rebuilds them, the JSON says per
entry what its library was.  `final_form` and `whole_step` are this tree.

    python profiles/pair_epilogue_ab.py launches --parent-lib LIB --out FILE [--rounds 2] [--more NAME=LIB,...]
        per launch and per gradient evaluation: a child process per library, parent and this tree alternating.  A child times the ten
        launch shapes of profiles/r05_pair_knockouts.txt and layer2's 3 x 3 (200704 x 1152 -> 128) on the tiles gp_plan chooses, the
        three C = 64 instances of the layer1 tail kernel (NEXT, NEXT + XS, plain; forward form), and one reference-precision gradient
        evaluation at B = 256.  --more: further libraries (lab builds) that take their turn after the two
    python profiles/pair_epilogue_ab.py step --parent DIR --out FILE [--rounds 4] [--key whole_step]
        bench.py --gpus 1 --steps 20 --warmup 5, a checkout of the parent commit (library built) and this tree alternating in child
        processes; round 0 with --dump-outputs on both sides, every array compared with numpy.array_equal

Both modes merge their result into FILE.  Operands are random; a launch's time does not depend on their values."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
GP_RELU = 1
# M_K_N_taps -> (batch, h, w, channels per tap, N, taps, skip pair in the epilogue): the shapes of r05_pair_knockouts.txt + layer2's 3 x 3
SHAPES = {'50176_256_1024_1': (256, 14, 14, 256, 1024, 1, True), '50176_1024_256_1': (256, 14, 14, 1024, 256, 1, False),
          '50176_2304_256_9': (256, 14, 14, 256, 256, 9, False), '802816_256_64_1': (256, 56, 56, 256, 64, 1, False),
          '802816_64_256_1': (256, 56, 56, 64, 256, 1, False), '12544_4608_512_9': (256, 7, 7, 512, 512, 9, False),
          '200704_128_512_1': (256, 28, 28, 128, 512, 1, True), '200704_512_128_1': (256, 28, 28, 512, 128, 1, False),
          '12544_512_2048_1': (256, 7, 7, 512, 2048, 1, True), '12544_2048_512_1': (256, 7, 7, 2048, 512, 1, False),
          '200704_1152_128_9': (256, 28, 28, 128, 128, 9, False)}


def time_entry(fn, d, reps=10, warm=2):
    import torch
    from robustart_amd import _lib
    for _ in range(warm):
        _lib.check(fn(ctypes.byref(d), _lib.stream_ptr()))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        _lib.check(fn(ctypes.byref(d), _lib.stream_ptr()))
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / reps * 1e3, 1)


def launch_us(lib):
    """us per launch of every shape: bias (+ skip pair) + ReLU + sign bytes, the tiles of the plan"""
    import torch
    from robustart_amd.model.engine_base import gemm_pair_desc, pair
    g = torch.Generator(device='cuda').manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device='cuda')
    out = {}
    for name, (b, h, w, c, n, taps, skip) in SHAPES.items():
        m, k = b * h * w, c * taps
        a, wp = pair(r(m, c)), pair(r(n, k) * 0.05)
        tab = torch.cat([wp[0], wp[1], wp[0]], 1).contiguous()
        dst = torch.empty(2, m, n, dtype=torch.bfloat16, device='cuda')
        sign = torch.empty(m * n // 8, dtype=torch.uint8, device='cuda')
        res = pair(r(m, n)) if skip else None
        tp = [(0, 0)] if taps == 1 else [(i // 3 - 1, i % 3 - 1) for i in range(9)]
        d = gemm_pair_desc(a, tab, dst, n, c, 3 * k, n, n, bias=r(n), res=res, sign_out=sign, flags=GP_RELU, w_lo_off=k, batch=b, grid=(h, w),
                           src_hw=(h, w), k_per_tap=c, taps=tp, dst_hw=(h, w))
        out[name] = sorted(time_entry(lib.rart_gemm_pair_bf16, d) for _ in range(3))
        del a, wp, tab, dst, sign, res, d
    return out


def tail_us(lib):
    """us per call of the three C = 64 instances the engine launches in layer1 (B = 256, 56 x 56), forward form"""
    import torch
    from robustart_amd import _lib
    B, H, C, N = 256, 56, 64, 256
    P = B * H * H
    pt = lambda *s: (torch.randn(2, *s, device='cuda') * 0.5).to(torch.bfloat16)
    src, dst, res, dstn, x = pt(P, C), pt(P, N), pt(P, N), pt(P, C), pt(P, C)
    tab = (torch.randn(C, 3 * 9 * C, device='cuda') * 0.05).to(torch.bfloat16)
    tail, ntab, tx = pt(N * C) * 0.1, pt(N * C) * 0.1, pt(N * C) * 0.1
    b2, b3, bn = torch.randn(C, device='cuda'), torch.randn(N, device='cuda'), torch.randn(C, device='cuda')
    sm, so, sn = (torch.zeros(P, c // 8, dtype=torch.uint8, device='cuda') for c in (C, N, C))
    out = {}
    for name, nxt, xs in (('next', 1, 0), ('next_xs', 1, 1), ('plain', 0, 0)):
        d = _lib.ConvTailDesc()
        d.a_hi, d.a_lo, d.w_hi, d.w_lo = src[0].data_ptr(), src[1].data_ptr(), tab.data_ptr(), tab.data_ptr() + 2 * 9 * C
        d.t_hi, d.t_lo, d.dst_hi, d.dst_lo = tail[0].data_ptr(), tail[1].data_ptr(), dst[0].data_ptr(), dst[1].data_ptr()
        d.batch, d.h, d.w, d.c_mid, d.ldw = B, H, H, C, 3 * 9 * C
        for i in range(9):
            d.tap_dy[i], d.tap_dx[i] = i // 3 - 1, i % 3 - 1
        if xs:
            d.x_hi, d.x_lo, d.tx_hi, d.tx_lo = x[0].data_ptr(), x[1].data_ptr(), tx[0].data_ptr(), tx[1].data_ptr()
        else:
            d.res_hi, d.res_lo = res[0].data_ptr(), res[1].data_ptr()
        d.bias_mid, d.bias_out, d.sign_mid, d.sign_out = b2.data_ptr(), b3.data_ptr(), sm.data_ptr(), so.data_ptr()
        d.relu_mid = d.relu_out = 1
        if nxt:
            d.n_hi, d.n_lo, d.dstn_hi, d.dstn_lo = ntab[0].data_ptr(), ntab[1].data_ptr(), dstn[0].data_ptr(), dstn[1].data_ptr()
            d.bias_next, d.sign_next, d.relu_next = bn.data_ptr(), sn.data_ptr(), 1
        out[name] = sorted(time_entry(lib.rart_conv3x3_tail_pair, d) for _ in range(3))
    return out


def grad_ms():
    """ms per reference-precision gradient evaluation at B = 256: three back to back, three times, after one round of warm-up"""
    import torch
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import ResNet50Engine
    torch.manual_seed(0)
    eng = ResNet50Engine(get_model({'type': 'resnet50_official'}).eval(), 'cuda', 'fp32x')
    x = torch.rand(256, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (256,), device='cuda')
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    ms = []
    for r in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            eng.forward_backward(x, mean, std, y, 0)
        e1.record()
        torch.cuda.synchronize()
        if r:
            ms.append(round(e0.elapsed_time(e1) / 3, 3))
    return sorted(ms)


def child(lib_path):
    from robustart_amd import _lib
    if lib_path != 'product':
        _lib.LIB_PATH = os.path.abspath(lib_path)
    lib = _lib.load()
    print(json.dumps({'launch_us': launch_us(lib), 'tail_us': tail_us(lib), 'grad_eval_ms': grad_ms()}))


def merge(out_path, key, value):
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc[key] = value
    json.dump(doc, open(out_path, 'w'), indent=1)


def launches(parent_lib, out_path, rounds, more=(), key='per_launch_and_gradient_evaluation'):
    sides = [('parent', os.path.abspath(parent_lib)), ('new', 'product')] + [(n, os.path.abspath(l)) for n, l in more]
    runs = {k: [] for k, _ in sides}
    for r in range(rounds):
        for name, lib in sides:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), 'child', '--lib', lib], capture_output=True, text=True, timeout=280)
            if p.returncode != 0:            # a child that failed ends the job: nothing more is started on the GPU
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit('child failed on %s (round %d, exit %d)' % (name, r, p.returncode))
            runs[name].append(json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1]))
            print(name, r, runs[name][-1], flush=True)
    med = {}
    for part in ('launch_us', 'tail_us'):
        for k in runs['parent'][0][part]:
            m = {s: statistics.median([v for run in runs[s] for v in run[part][k]]) for s in runs}
            med['%s %s' % (part, k)] = dict(m, gain_percent={s: round(100 * (m['parent'] - m[s]) / m['parent'], 1) for s in m if s != 'parent'})
    m = {s: statistics.median([v for run in runs[s] for v in run['grad_eval_ms']]) for s in runs}
    med['grad_eval_ms'] = dict(m, gain_percent={s: round(100 * (m['parent'] - m[s]) / m['parent'], 2) for s in m if s != 'parent'})
    merge(out_path, key, {
        'what': 'B = 256 shapes on one MI355X; a child process per library, the libraries taking turns, %d per side.  launch_us: us per '
                'launch (ten back to back after two, three groups, sorted) of rart_gemm_pair_bf16 with bias (+ skip pair where the layer has one) + '
                'ReLU + sign bytes on the tiles of the plan; tail_us: the same for the C = 64 instances of rart_conv3x3_tail_pair (forward form); '
                'grad_eval_ms: ResNet50Engine(fp32x).forward_backward, three back to back, three groups' % rounds,
        'runs': runs, 'medians': med})
    print(json.dumps(med, indent=1))


def step_ab(parent, out_path, rounds, key='whole_step'):
    """the headline step, parent tree (library built) against this tree, alternating in child processes; round 0 dumps the outputs"""
    import numpy as np
    trees = [('parent', os.path.abspath(parent)), ('new', HERE)]
    tmp = tempfile.mkdtemp()
    runs = {k: [] for k, _ in trees}
    for r in range(rounds):
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
            print(name, r, round(j['ms_per_step'], 3), flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    gain, bar = med['parent'] - med['new'], 3 * max(spread.values())
    outs = {}
    for f in sorted(os.listdir(os.path.join(tmp, 'parent'))):
        outs[f] = bool(np.array_equal(np.load(os.path.join(tmp, 'parent', f)), np.load(os.path.join(tmp, 'new', f))))
    below = max(runs['new']) < min(runs['parent'])
    res = {'what': 'headline bench, reference precision, B = 256, one MI355X: the parent commit against this tree',
           'command': 'python bench.py --gpus 1 --steps 20 --warmup 5 (one job, the two trees alternating in child processes, %d runs per side); '
                      'round 0 with --dump-outputs DIR on both sides' % rounds,
           'ms_per_step': runs, 'median_ms_per_step': med, 'spread_max_minus_min_ms': spread, 'gain_ms_per_step': gain,
           'gain_percent': 100 * gain / med['parent'], 'bar_ms': bar, 'every_new_run_below_every_parent_run': below,
           'clears_the_bar': bool(below and gain > bar), 'outputs_array_equal': outs, 'n_outputs': len(outs)}
    merge(out_path, key, res)
    print(json.dumps({k: res[k] for k in ('ms_per_step', 'median_ms_per_step', 'spread_max_minus_min_ms', 'gain_ms_per_step', 'bar_ms', 'clears_the_bar')}))
    print('outputs array_equal:', all(outs.values()), len(outs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['launches', 'child', 'step'])
    ap.add_argument('--out')
    ap.add_argument('--lib', default='product')
    ap.add_argument('--parent-lib')
    ap.add_argument('--parent')
    ap.add_argument('--rounds', type=int, default=0)
    ap.add_argument('--more', default='')
    ap.add_argument('--key', default='')
    a = ap.parse_args()
    if a.mode == 'child':
        return child(a.lib)
    if a.mode == 'launches':
        return launches(a.parent_lib, a.out, a.rounds or 2, [kv.split('=', 1) for kv in a.more.split(',') if kv], a.key or 'per_launch_and_gradient_evaluation')
    return step_ab(a.parent, a.out, a.rounds or 4, a.key or 'whole_step')


if __name__ == '__main__':
    main()
