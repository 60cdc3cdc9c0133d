"""Layer3's short-K pair expansions (50176 x 256 -> 1024 at B = 256): what keeping the A rows resident can return, and the A/Bs of
rart_expand_walk_pair against rart_gemm_pair_bf16.  Every figure of profiles/expand_walk_ab.json comes from one of these modes:

    python profiles/expand_walk_ab.py ko-build                   (no GPU) the knock-out library: k_gemm_pair's A stage loads issued by
                                                                 column tile 0 only (MFMAs on stale tiles; timing only)
    python profiles/expand_walk_ab.py bounds --out FILE          the two layer3 descriptors and layer2's twin replayed on the product library
                                                                 and on the knock-out library, at M = 50176 and M = 192 x 256, forced tiles
    python profiles/expand_walk_ab.py kernel --out FILE          old entry against new, alternating, three groups of ten, bit for bit
    python profiles/expand_walk_ab.py grad --out FILE [--channels 256,128]
                                                                 one gradient evaluation at B = 256, engine switch off / on, alternating
    python profiles/expand_walk_ab.py step --parent DIR --out FILE [--rounds 4]
                                                                 bench.py --gpus 1 --steps 20 --warmup 5, parent tree and this tree alternating
                                                                 in child processes; round 0 with --dump-outputs on both sides

The descriptors are the two that `ResNet50Engine.forward_backward` issues for an identity block of layer3: the expansion (bias + skip pair
+ ReLU + sign bytes) and conv1^T (no bias, the gradient pair as residual, a 1-bit mask).  Operands are random; a 1x1 launch's time does not
depend on their values."""
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
KO_DIR = os.path.join(HERE, 'scratch', 'exp', '_bin', 'expand_walk_ko')
KO_LIB = os.path.join(KO_DIR, 'librobustart_hip_a_once.so')
GP_RELU = 1
SHAPES = {'layer3': (50176, 256, 1024), 'layer3_6_passes': (192 * 256, 256, 1024), 'layer2_twin': (200704, 128, 512)}


def ko_build():
    """the product library with gemm_pair.o replaced by a build of the PRODUCT source in which only column tile 0 issues the A stage loads
    of a one-tap launch (two patched lines, no second copy of the kernel)"""
    src = os.path.join(HERE, 'robustart_amd', 'csrc', 'gemm_pair.hip')
    text = open(src).read()
    n = 0
    for plane in ('srd_ah', 'srd_al'):
        old = 'rart_dma_load16(avoff[q], %s, so_,' % plane
        n += text.count(old)
        text = text.replace(old, 'if (n_tile == 0) rart_dma_load16(avoff[q], %s, so_,' % plane)
    assert n == 2, 'the knock-out patch did not apply'
    os.makedirs(KO_DIR, exist_ok=True)
    patched = os.path.join(KO_DIR, 'gemm_pair_a_once.hip')
    open(patched, 'w').write(text)
    obj_dir = os.path.join(HERE, 'robustart_amd', 'csrc', '_obj')
    objs = sorted(os.path.join(obj_dir, f) for f in os.listdir(obj_dir) if f.endswith('.o') and not f.startswith('gemm_pair.hip'))
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    o = os.path.join(KO_DIR, 'gemm_pair_a_once.o')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I', os.path.join(HERE, 'include'),
                    '-I', os.path.join(HERE, 'robustart_amd', 'csrc'), '-c', patched, '-o', o], check=True)
    subprocess.run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', KO_LIB] + objs + [o], check=True)
    print('built', KO_LIB)


def operands(M, K, N, seed=0):
    import torch
    from robustart_amd.model.engine_base import pair
    g = torch.Generator(device='cuda').manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device='cuda')
    w = pair(r(N, K) * 0.05)
    return dict(M=M, K=K, N=N, a=pair(r(M, K)), tab=torch.cat([w[0], w[1], w[0]], 1).contiguous(), bias=r(N), res=pair(r(M, N)),
                mask=torch.randint(0, 256, (M * N // 8,), generator=g, device='cuda', dtype=torch.uint8))


def descriptor(c, form, dst, sign=None, tile=(0, 0), grid=None):
    """form 'fwd': bias + skip pair + ReLU (+ sign bytes); 'bwd': residual pair + 1-bit mask.  The rows as one image of M x 1 pixels
    unless `grid` = (batch, h, w) says otherwise"""
    from robustart_amd.model.engine_base import gemm_pair_desc
    b, h, w = grid or (1, c['M'], 1)
    fwd = form == 'fwd'
    return gemm_pair_desc(c['a'], c['tab'], dst, c['N'], c['K'], 3 * c['K'], c['N'], c['N'], bias=c['bias'] if fwd else None, res=c['res'],
                          mask_bits=None if fwd else c['mask'], sign_out=sign if fwd else None, flags=GP_RELU if fwd else 0,
                          w_lo_off=c['K'], batch=b, grid=(h, w), src_hw=(h, w), k_per_tap=c['K'], taps=[(0, 0)], dst_hw=(h, w), tile=tile)


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


def bounds_child(lib_path):
    """us per launch of every shape, form and forced tile on one library"""
    import torch
    from robustart_amd import _lib
    if lib_path != 'product':
        _lib.LIB_PATH = lib_path
    lib = _lib.load()
    out = {}
    for name, (M, K, N) in SHAPES.items():
        c = operands(M, K, N)
        dst = torch.empty(2, M, N, dtype=torch.bfloat16, device='cuda')
        sign = torch.empty(M * N // 8, dtype=torch.uint8, device='cuda')
        for form in ('fwd', 'bwd'):
            for tile in ((0, 0), (128, 64), (256, 128)):
                out['%s_%s_tile%dx%d' % (name, form, tile[0], tile[1])] = time_entry(lib.rart_gemm_pair_bf16, descriptor(c, form, dst, sign, tile))
        del c, dst, sign
    print(json.dumps(out))


def bounds(out_path):
    res = {}
    for name, lib in (('product', 'product'), ('a_loads_by_column_tile_0_only', KO_LIB), ('product_again', 'product')):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), 'bounds-child', '--lib', lib], capture_output=True, text=True, timeout=240)
        if p.returncode != 0:            # a child that failed ends the job: nothing more is started on the GPU
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit('bounds child failed on %s (exit %d)' % (name, p.returncode))
        res[name] = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
        print(name, res[name], flush=True)
    k = 'layer3_%s_tile0x0'
    summary = {}
    for form in ('fwd', 'bwd'):
        base = min(res['product'][k % form], res['product_again'][k % form])
        ko = res['a_loads_by_column_tile_0_only'][k % form]
        summary[form] = {'us_product': base, 'us_a_loaded_once': ko, 'bound_us': round(base - ko, 1), 'bound_percent': round(100 * (base - ko) / base, 1),
                         'us_192x256_rows': res['product']['layer3_6_passes_%s_tile0x0' % form],
                         'us_layer2_twin': res['product']['layer2_twin_%s_tile0x0' % form]}
    json.dump({'what': 'us per launch, B = 256 shapes, ten launches back to back after two; tile0x0 = the tile policy\'s choice (256 x 64)',
               'shapes_M_K_N': SHAPES, 'us_per_launch': res, 'layer3': summary,
               'stop_rule': 'stop if the bound is under 10 % of the launch (14 us)'}, open(out_path, 'w'), indent=1)
    print(json.dumps(summary))


def kernel_ab(out_path):
    """both descriptors at layer3's shape (and layer2's twin), old entry against new at both row tiles, alternating: three groups of ten
    launches per side; the outputs compared bit for bit"""
    import torch
    from robustart_amd import _lib
    lib = _lib.load()
    res = {}
    for name in ('layer3', 'layer2_twin'):
        M, K, N = SHAPES[name]
        c = operands(M, K, N)
        outs = [(torch.empty(2, M, N, dtype=torch.bfloat16, device='cuda'), torch.empty(M * N // 8, dtype=torch.uint8, device='cuda')) for _ in range(2)]
        for form in ('fwd', 'bwd'):
            old = lambda d, s: lib.rart_gemm_pair_bf16(d, s)
            walk = lambda tr, parts: (lambda d, s: lib.rart_expand_walk_pair(d, tr, parts, s), 1)
            sides = {'gemm_pair': (old, 0), 'walk_128': walk(128, 1), 'walk_128_2_parts': walk(128, 2), 'walk_128_4_parts': walk(128, 4),
                     'walk_64': walk(64, 1), 'walk_64_2_parts': walk(64, 2)}
            for o in outs:
                o[0].fill_(float('nan')), o[1].fill_(0xA5)
            us = {k: [] for k in sides}
            for _ in range(3):
                for k, (fn, slot) in sides.items():
                    us[k].append(time_entry(fn, descriptor(c, form, outs[slot][0], outs[slot][1]), reps=10, warm=1))
            equal = {}
            for k in [k for k in sides if k != 'gemm_pair']:      # (the sides share slot 1: run each once more for the comparison)
                outs[1][0].fill_(float('nan')), outs[1][1].fill_(0xA5)
                time_entry(sides[k][0], descriptor(c, form, outs[1][0], outs[1][1]), reps=1, warm=0)
                equal[k] = bool(torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)) and torch.equal(outs[0][1], outs[1][1]))
            res['%s_%s' % (name, form)] = {'us_per_launch_groups_of_10': us, 'median_us': {k: statistics.median(v) for k, v in us.items()},
                                           'hi_lo_sign_bit_equal_to_gemm_pair': equal}
            print(name, form, res['%s_%s' % (name, form)], flush=True)
        del c, outs
    json.dump({'what': 'kernel alone, B = 256 shapes: rart_gemm_pair_bf16 (tile policy) against rart_expand_walk_pair at 128- and 64-row tiles, the columns of a row tile in 1 / 2 / 4 workgroups',
               'shapes_M_K_N': SHAPES, 'results': res}, open(out_path, 'w'), indent=1)


def grad_ab(out_path, channels):
    """one reference-precision gradient evaluation at B = 256, `expand_walk_pair` off / on alternating, five pairs; channels: the
    engine's `expand_walk_channels` of the run (the K widths that take the new entry)"""
    import torch
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import ResNet50Engine
    torch.manual_seed(0)
    eng = ResNet50Engine(get_model({'type': 'resnet50_official'}).eval(), 'cuda', 'fp32x')
    eng.expand_walk_channels = tuple(channels)
    x = torch.rand(256, 3, 224, 224, device='cuda')
    y = torch.randint(0, 1000, (256,), device='cuda')
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    ms, outs = {False: [], True: []}, {}
    for r in range(6):
        for on in (False, True):
            eng.expand_walk_pair = on
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                o = eng.forward_backward(x, mean, std, y, 0)
            e1.record()
            torch.cuda.synchronize()
            if r:                       # round 0 warms both sides up
                ms[on].append(round(e0.elapsed_time(e1) / 3, 3))
            outs[on] = (o[0].clone(), o[2].clone())
    res = {'what': 'ResNet50Engine(fp32x).forward_backward at B = 256, ms per gradient evaluation (three back to back), switch alternating',
           'expand_walk_channels': list(channels),
           'ms_off': ms[False], 'ms_on': ms[True], 'median_off': statistics.median(ms[False]), 'median_on': statistics.median(ms[True]),
           'logits_and_input_gradient_bit_equal': bool(torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[False][1], outs[True][1]))}
    json.dump(res, open(out_path, 'w'), indent=1)
    print(json.dumps(res))


def step_ab(parent, out_path, rounds):
    """the headline step, parent tree (library built) against this tree, alternating in child processes; round 0 dumps the outputs"""
    import numpy as np
    trees = [('parent', os.path.abspath(parent)), ('walk', HERE)]
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
    gain, bar = med['parent'] - med['walk'], 3 * max(spread.values())
    outs = {}
    for f in sorted(os.listdir(os.path.join(tmp, 'parent'))):
        outs[f] = bool(np.array_equal(np.load(os.path.join(tmp, 'parent', f)), np.load(os.path.join(tmp, 'walk', f))))
    below = max(runs['walk']) < min(runs['parent'])
    res = {'what': 'headline bench, reference precision, B = 256, one MI355X: the parent commit against this tree',
           'command': 'python bench.py --gpus 1 --steps 20 --warmup 5 (one job, the two trees alternating in child processes, %d runs per side); '
                      'round 0 with --dump-outputs DIR on both sides' % rounds,
           'ms_per_step': runs, 'median_ms_per_step': med, 'spread_max_minus_min_ms': spread, 'gain_ms_per_step': gain,
           'gain_percent': 100 * gain / med['parent'], 'bar_ms': bar, 'every_walk_run_below_every_parent_run': below,
           'clears_the_bar': bool(below and gain > bar), 'outputs_array_equal': outs, 'n_outputs': len(outs)}
    json.dump(res, open(out_path, 'w'), indent=1)
    print(json.dumps({k: res[k] for k in ('median_ms_per_step', 'spread_max_minus_min_ms', 'gain_ms_per_step', 'bar_ms', 'clears_the_bar')}))
    print('outputs array_equal:', all(outs.values()), len(outs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['ko-build', 'bounds', 'bounds-child', 'kernel', 'grad', 'step'])
    ap.add_argument('--out')
    ap.add_argument('--lib', default='product')
    ap.add_argument('--parent')
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--channels', default='256')
    a = ap.parse_args()
    if a.mode == 'ko-build':
        return ko_build()
    if a.mode == 'bounds-child':
        return bounds_child(a.lib)
    if a.mode == 'bounds':
        return bounds(a.out)
    if a.mode == 'kernel':
        return kernel_ab(a.out)
    if a.mode == 'grad':
        return grad_ab(a.out, [int(c) for c in a.channels.split(',')])
    return step_ab(a.parent, a.out, a.rounds)


if __name__ == '__main__':
    main()
