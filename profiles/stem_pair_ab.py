"""A/B of builds of the library on the three fused pair stem kernels alone and on the whole bench.py step (one MI355X).

    python profiles/stem_pair_ab.py kernels LIB_A.so LIB_B.so ... [--rounds 2]     per-launch times (B = 256, 224 x 224), device events
    python profiles/stem_pair_ab.py bench   LIB_A.so LIB_B.so [--rounds 4] [--dump DIR]   bench.py --steps 20 --warmup 5 per build
The builds alternate in child processes, so box-to-box and warm-up effects cancel.  `bench` with --dump writes the --dump-outputs
arrays of the first round per build under DIR/<n> and compares them with numpy.array_equal.  Other builds come from
profiles/stem_pair_lab_build.py."""
import ctypes, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if sys.argv[1] == '--kernels-child':
    from robustart_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[2])
    import torch
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.model.engine_base import pair
    lib = _lib.load()
    B, H, W = 256, 224, 224
    g = torch.Generator().manual_seed(5)
    wb = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    wt = pair(ResNet50Engine._stem_bwd_table(wb, dtype=torch.float32)).cuda()
    rows = torch.zeros(64, 7, 8, 4); rows[:, :, :7, :3] = wb.permute(0, 2, 3, 1)
    wf = pair(rows.reshape(64, 224)).cuda()
    bias = torch.randn(64, generator=g).cuda()
    xf = torch.rand(B, 3, H, W, generator=g).cuda()
    xu = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    p1 = torch.empty(2, B, H // 4, W // 4, 64, dtype=torch.bfloat16, device='cuda')
    arg = torch.empty(B, H // 4, W // 4, 64, dtype=torch.uint8, device='cuda')
    sign = torch.empty(B, H // 4, W // 4, 8, dtype=torch.uint8, device='cuda')
    dp = pair(torch.randn(B, H // 4, W // 4, 64, generator=g)).cuda()
    grad = torch.empty(B, 3, H, W, device='cuda')
    m3 = (ctypes.c_float * 3)(0.485, 0.456, 0.406); s3 = (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    sp = _lib.stream_ptr()
    fwd = lambda x, u8: _lib.check(lib.rart_engine_stem_fwd_fused_pair(_lib.ptr(x), u8, _lib.ptr(wf[0]), _lib.ptr(wf[1]), _lib.ptr(bias), _lib.ptr(p1[0]), _lib.ptr(p1[1]), _lib.ptr(arg), _lib.ptr(sign), B, H, W, m3, s3, sp))
    bwd = lambda: _lib.check(lib.rart_engine_stem_bwd_fused_pair(_lib.ptr(dp[0]), _lib.ptr(dp[1]), _lib.ptr(arg), _lib.ptr(wt[0]), _lib.ptr(wt[1]), _lib.ptr(grad), B, H, W, s3, sp))
    def t(fn, n=30):
        for _ in range(5): fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): fn()
        e1.record(); torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / n * 1e3, 1)
    print(json.dumps({'lib': sys.argv[2], 'fwd_f32_us': t(lambda: fwd(xf, 0)), 'fwd_u8_us': t(lambda: fwd(xu, 1)), 'bwd_us': t(bwd)}), flush=True)
    sys.exit(0)
if sys.argv[1] == '--bench-child':
    import runpy
    from robustart_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[2])
    sys.argv = [os.path.join(ROOT, 'bench.py')] + sys.argv[3:]
    runpy.run_path(sys.argv[0], run_name='__main__')
    sys.exit(0)

mode, args = sys.argv[1], sys.argv[2:]
rounds = int(args[args.index('--rounds') + 1]) if '--rounds' in args else (2 if mode == 'kernels' else 4)
dump = args[args.index('--dump') + 1] if '--dump' in args else None
libs = [a for a in args if a.endswith('.so')]
for r in range(rounds):
    for n, lib in enumerate(libs):
        if mode == 'kernels':
            cmd = [sys.executable, os.path.abspath(__file__), '--kernels-child', lib]
        else:
            cmd = [sys.executable, os.path.abspath(__file__), '--bench-child', lib, '--gpus', '1', '--steps', '20', '--warmup', '5']
            if dump and r == 0:
                cmd += ['--dump-outputs', os.path.join(dump, str(n))]
        o = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        line = [ln for ln in o.stdout.splitlines() if ln.startswith('{')]
        if o.returncode != 0 or not line:
            sys.exit('child failed for %s:\n%s' % (lib, o.stderr[-2000:]))
        j = json.loads(line[-1])
        print(json.dumps(j if mode == 'kernels' else {'lib': lib, 'round': r, 'ms_per_step': j['ms_per_step'], 'value': j['value']}), flush=True)
if mode == 'bench' and dump:
    import numpy as np
    a, b = os.path.join(dump, '0'), os.path.join(dump, '1')
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b))
    bad = [n for n in names if not np.array_equal(np.load(os.path.join(a, n)), np.load(os.path.join(b, n)))]
    print(json.dumps({'dump_outputs_arrays': len(names), 'array_equal': not bad, 'different': bad}), flush=True)
    sys.exit(1 if bad else 0)
