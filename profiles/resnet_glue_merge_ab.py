"""The merge of the ResNet-50 glue kernels (csrc/engine_aux.hip) and of the two unpatchify kernels (csrc/vit_bwd.hip), parent commit
against this tree.  Three parts, each writes its own key of profiles/resnet_glue_merge_ab.json and leaves the others alone:

    python profiles/resnet_glue_merge_ab.py resources --parent-tree DIR          (no GPU: compiles both trees' glue sources)
    python profiles/resnet_glue_merge_ab.py entries   --parent-tree DIR          (one GPU)
    python profiles/resnet_glue_merge_ab.py headline  --parent-tree DIR [--pairs 3]

DIR is a checkout of the parent commit with its library built (robustart_amd/lib/librobustart_hip.so).

resources: `hipcc -Rpass-analysis=kernel-resource-usage` on the sources that hold the merged kernels; per kernel instance VGPRs, LDS
bytes, scratch and occupancy, parent beside new.
entries: both libraries are loaded into ONE process and alternate parent, new, parent, new, ...; a repeat is a window of at least
--window seconds of back-to-back calls of one entry between two device events, at the headline workload's shapes (B = 256).  An entry
passes when the new median is no worse than the parent median by more than the parent's own spread (max - min of its repeats).
`entries --new-lib COPY_OF_THE_PARENT_LIBRARY --key entries_null` is the null experiment: the same code loaded twice.
headline: `bench.py --gpus 1 --steps 20 --warmup 5` in a fresh process per run, the two trees alternating; the new median ms_per_step
must lie within the range of the parent's repeats."""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'resnet_glue_merge_ab.json')
LIB = os.path.join('robustart_amd', 'lib', 'librobustart_hip.so')
STD = (0.229, 0.224, 0.225)
B = 256


def merge_out(path, key, value):
    res = json.load(open(path)) if os.path.exists(path) else {}
    res[key] = value
    with open(path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


# ------------------------------------------------------------------ resources
SOURCES = {'parent': ('engine_aux.hip', 'engine_aux_pair.hip', 'vit_bwd.hip', 'vit_pair.hip'), 'new': ('engine_aux.hip', 'vit_bwd.hip')}
KERNELS = re.compile(r'k_(maxpool|avgpool|f32_to|stem_col2im|unpatchify)')
FIELDS = {'VGPRs': 'vgprs', 'ScratchSize [bytes/lane]': 'scratch', 'Occupancy [waves/SIMD]': 'occupancy', 'LDS Size [bytes/block]': 'lds_static'}


def resource_usage(tree, which):
    from robustart_amd.csrc import build as b
    out = {}
    for src in SOURCES[which]:
        cmd = [b.HIPCC] + b.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(tree, 'robustart_amd', 'csrc', src),
                                     '-o', os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        name = None
        for line in text.splitlines():
            m = re.search(r'remark: Function Name: (\S+)', line)
            if m:
                name = subprocess.run(['c++filt', m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
                name = re.sub(r'\(.*$', '', re.sub(r'^(void )?\(anonymous namespace\)::', '', name)) if KERNELS.search(name) else None
                if name:
                    out[name] = {'source': src}
            m = re.search(r'remark:\s+([A-Za-z \[\]/]+): (\d+)', line)
            if m and name and m.group(1) in FIELDS:
                out[name][FIELDS[m.group(1)]] = int(m.group(2))
    return out


def run_resources(a):
    res = {'parent': resource_usage(a.parent_tree, 'parent'), 'new': resource_usage(ROOT, 'new'),
           'note': 'lds_static and occupancy are what the compiler reports.  Every instance has the VGPRs, static LDS, scratch (0) and occupancy of the parent kernel it replaces.  The fp32 col2im takes its 11 * 19 * 152 * 4 = 127 072 B of LDS at launch, before and after, so its reported occupancy of 8 is on paper: one workgroup of sixteen waves per CU.'}
    merge_out(a.out, 'resources', res)
    for which in ('parent', 'new'):
        for k, v in res[which].items():
            print(which, k, v)


# ------------------------------------------------------------------ entries
def load(path):
    import torch  # noqa: F401  (its HIP runtime first, as robustart_amd._lib.load does)
    from robustart_amd import _lib as L
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.rart_version() == L.ABI_VERSION
    return lib


def entry_calls(L, sp):
    """-> {entry: (make, call)}: make() allocates the operands at the workload's shape, call(lib, operands) issues the entry once"""
    import torch
    bf, f32, u8 = torch.bfloat16, torch.float32, torch.uint8
    dev = 'cuda'
    std = (ctypes.c_float * 3)(*STD)

    def randn(*shape, dtype=bf):
        return torch.randn(*shape, device=dev, dtype=f32).to(dtype)

    def pair(*shape):
        v = torch.randn(*shape, device=dev)
        hi = v.to(bf)
        return torch.stack([hi, (v - hi.float()).to(bf)]).contiguous()

    def zeros(*shape, dtype=bf):
        return torch.zeros(*shape, device=dev, dtype=dtype)
    p = L.ptr
    H, C, HW, CF = 112, 64, 49, 2048
    cases = {}
    # max pool 112 x 112 x 64 -> 56 x 56; the backward on the forward's own codes
    def mp_fwd():
        return dict(x=randn(B, H, H, C).relu_(), out=zeros(B, H // 2, H // 2, C), arg=zeros(B, H // 2, H // 2, C, dtype=u8),
                    sign=zeros(B, H // 2, H // 2, C // 8, dtype=u8))
    cases['rart_engine_maxpool_keep'] = (mp_fwd, lambda lib, o: lib.rart_engine_maxpool_keep(p(o['x']), p(o['out']), p(o['arg']), p(o['sign']), B, H, H, C, sp))

    def mp_fwd_pair():
        return dict(x=pair(B, H, H, C).relu_(), out=zeros(2, B, H // 2, H // 2, C), arg=zeros(B, H // 2, H // 2, C, dtype=u8),
                    sign=zeros(B, H // 2, H // 2, C // 8, dtype=u8))
    cases['rart_engine_maxpool_pair'] = (mp_fwd_pair, lambda lib, o: lib.rart_engine_maxpool_pair(
        p(o['x']), o['x'][0].numel(), p(o['out']), o['out'][0].numel(), p(o['arg']), p(o['sign']), B, H, H, C, sp))

    def mp_bwd():
        o = mp_fwd()
        L.check(cases['rart_engine_maxpool_keep'][1](L.load(), o))
        return dict(y=o['x'], arg=o['arg'], dp=randn(B, H // 2, H // 2, C), dz=zeros(B, H, H, C))
    cases['rart_engine_maxpool_bwd'] = (mp_bwd, lambda lib, o: lib.rart_engine_maxpool_bwd(p(o['y']), p(o['arg']), p(o['dp']), p(o['dz']), B, H, H, C, sp))

    def mp_bwd_pair():
        o = mp_fwd_pair()
        L.check(cases['rart_engine_maxpool_pair'][1](L.load(), o))
        return dict(arg=o['arg'], dp=pair(B, H // 2, H // 2, C), dz=zeros(2, B, H, H, C))
    cases['rart_engine_maxpool_bwd_pair'] = (mp_bwd_pair, lambda lib, o: lib.rart_engine_maxpool_bwd_pair(
        p(o['arg']), p(o['dp']), o['dp'][0].numel(), p(o['dz']), o['dz'][0].numel(), B, H, H, C, sp))
    # global average pool 49 x 2048
    cases['rart_engine_avgpool'] = (lambda: dict(x=randn(B, HW, CF), out=zeros(B, CF)),
                                    lambda lib, o: lib.rart_engine_avgpool(p(o['x']), p(o['out']), B, HW, CF, sp))
    cases['rart_engine_avgpool_pair'] = (lambda: dict(x=pair(B, HW, CF), out=zeros(2, B, CF)), lambda lib, o: lib.rart_engine_avgpool_pair(
        p(o['x']), o['x'][0].numel(), p(o['out']), o['out'][0].numel(), B, HW, CF, sp))
    cases['rart_engine_avgpool_bwd'] = (lambda: dict(y=randn(B, HW, CF), dp=randn(B, CF), dz=zeros(B, HW, CF)),
                                        lambda lib, o: lib.rart_engine_avgpool_bwd(p(o['y']), p(o['dp']), p(o['dz']), B, HW, CF, sp))
    cases['rart_engine_avgpool_bwd_pair'] = (
        lambda: dict(sign=torch.randint(0, 256, (B, HW, CF // 8), device=dev, dtype=u8), dp=pair(B, CF), dz=zeros(2, B, HW, CF)),
        lambda lib, o: lib.rart_engine_avgpool_bwd_pair(p(o['sign']), p(o['dp']), o['dp'][0].numel(), p(o['dz']), o['dz'][0].numel(), B, HW, CF, sp))
    # dlogits 256 x 1000 -> rows of 1024
    cases['rart_f32_to_bf16_rows'] = (lambda: dict(src=randn(B, 1000, dtype=f32), dst=zeros(B, 1024)),
                                      lambda lib, o: lib.rart_f32_to_bf16_rows(p(o['src']), p(o['dst']), B, 1000, 1024, sp))
    cases['rart_f32_to_pair_rows'] = (lambda: dict(src=randn(B, 1000, dtype=f32), dst=zeros(2, B, 1024)),
                                      lambda lib, o: lib.rart_f32_to_pair_rows(p(o['src']), p(o['dst']), o['dst'][0].numel(), B, 1000, 1024, sp))
    # stem col2im to 224 x 224
    for name, dt in (('rart_engine_stem_col2im', bf), ('rart_engine_stem_col2im_f32', f32)):
        cases[name] = (lambda dt=dt: dict(pt=randn(B, 112, 112, 152, dtype=dt), g=zeros(B, 3, 224, 224, dtype=f32)),
                       lambda lib, o, name=name: getattr(lib, name)(p(o['pt']), p(o['g']), B, 224, 224, 152, std, sp))
    # unpatchify to 224 x 224: patch 16 (ViT, Mixer: row stride 768) in both patch types, patch 4 (ConvNeXt: row stride 64) in fp32
    for tag, name, dt, ps, ld in (('rart_vit_unpatchify_f32/patch16', 'rart_vit_unpatchify_f32', bf, 16, 768),
                                  ('rart_vit_unpatchify_from_f32/patch16', 'rart_vit_unpatchify_from_f32', f32, 16, 768),
                                  ('rart_vit_unpatchify_from_f32/patch4', 'rart_vit_unpatchify_from_f32', f32, 4, 64)):
        cases[tag] = (lambda dt=dt, ps=ps, ld=ld: dict(dp=randn(B * (224 // ps) ** 2, ld, dtype=dt), g=zeros(B, 3, 224, 224, dtype=f32)),
                      lambda lib, o, name=name, ps=ps, ld=ld: getattr(lib, name)(p(o['dp']), p(o['g']), B, 224, 224, ps, ld, std, sp))
    return cases


def run_entries(a):
    import torch
    from robustart_amd import _lib as L
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    libs = {'parent': load(os.path.join(a.parent_tree, LIB)), 'new': load(a.new_lib) if a.new_lib else L.load()}
    sp = L.stream_ptr()
    order = ['parent', 'new'] * a.repeats
    report = {}
    for entry, (make, call) in entry_calls(L, sp).items():
        ops = make()

        def window(lib, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                st = call(lib, ops)
            e1.record()
            e1.synchronize()
            L.check(st)
            return e0.elapsed_time(e1) * 1e3 / calls                     # us per call
        for lib in libs.values():
            window(lib, 10)                                              # warm-up: code objects, the dynamic-LDS attribute
        calls = max(10, int(a.window * 1e6 / window(libs['new'], 50)) + 1)
        us = {'parent': [], 'new': []}
        for which in order:
            us[which].append(window(libs[which], calls))
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = max(us['parent']) - min(us['parent'])
        report[entry] = dict(calls_per_window=calls, us_per_call=us, median_us=med, parent_spread_us=spread,
                             passes=med['new'] <= med['parent'] + spread)
        print(entry, json.dumps(report[entry]), flush=True)
        del ops
        torch.cuda.empty_cache()
    merge_out(a.out, a.key, dict(device=torch.cuda.get_device_name(0), batch=B, window_s=a.window, order=order, entries=report,
                                     all_pass=all(r['passes'] for r in report.values())))


# ------------------------------------------------------------------ headline
def run_headline(a):
    trees = {'parent': os.path.abspath(a.parent_tree), 'new': ROOT}
    order = ['parent', 'new'] * a.pairs
    ms, ips = {'parent': [], 'new': []}, {'parent': [], 'new': []}
    for which in order:
        r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '20', '--warmup', '5'], cwd=trees[which],
                           capture_output=True, text=True, timeout=a.bench_timeout)
        if r.returncode != 0:
            sys.exit('bench.py failed in the %s tree (exit %d):\n%s' % (which, r.returncode, r.stderr[-2000:]))
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
        ms[which].append(line['ms_per_step'])
        ips[which].append(line['value'])
        print(which, line['ms_per_step'], flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    rng = [min(ms['parent']), max(ms['parent'])]
    merge_out(a.out, 'headline', dict(what='bench.py --gpus 1 --steps 20 --warmup 5, a fresh process per run, the two trees alternating',
                                      order=order, ms_per_step=ms, images_per_s=ips, median_ms_per_step=med,
                                      parent_range_ms_per_step=rng, new_median_within_parent_range=rng[0] <= med['new'] <= rng[1],
                                      new_median_not_above_parent_range=med['new'] <= rng[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('part', choices=['resources', 'entries', 'headline'])
    ap.add_argument('--parent-tree', required=True)
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--repeats', type=int, default=4)
    ap.add_argument('--new-lib', default=None, help='entries: the library timed as "new" (default: this tree\'s).  A byte copy of the '
                    'parent\'s library here, with --key entries_null, measures what two loads of the SAME code differ by')
    ap.add_argument('--key', default='entries', help='entries: the key of the output file to write')
    ap.add_argument('--window', type=float, default=1.0, help='seconds of calls per repeat')
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--bench-timeout', type=int, default=240)
    a = ap.parse_args()
    dict(resources=run_resources, entries=run_entries, headline=run_headline)[a.part](a)


if __name__ == '__main__':
    main()
