"""Tile sweep of the fused (two-source) pair launches at B = 256 against the two launches they replace."""
import ctypes, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from robustart_amd import _lib
from robustart_amd.model.engine_base import gemm_pair_desc

lib = _lib.load()
sp = _lib.stream_ptr


def pairt(*shape):
    return (torch.randn(2, *shape, device='cuda') * 0.5).to(torch.bfloat16)


def launch(d):
    if isinstance(d, _lib.GemmPair2Desc):
        _lib.check(lib.rart_gemm_pair2_bf16(ctypes.byref(d), sp()))
    else:
        _lib.check(lib.rart_gemm_pair_bf16(ctypes.byref(d), sp()))


def timeit(descs, reps=8, groups=3):
    for _ in range(3):
        for d in descs:
            launch(d)
    torch.cuda.synchronize()
    ts = []
    for _ in range(groups):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            for d in descs:
                launch(d)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps * 1000)
    return sorted(ts)


B = 256
cases = [('layer2.0 fwd', 28, 128, 2, 256, 512, False), ('layer3.0 fwd', 14, 256, 2, 512, 1024, False), ('layer4.0 fwd', 7, 512, 2, 1024, 2048, False),
         ('layer1.0 bwd', 56, 64, 1, 256, 64, True)]
only = sys.argv[1:] 
for name, g, c1, s2, c2, n, bwd in cases:
    if only and not any(o in name for o in only):
        continue
    a1, a2 = pairt(B, g, g, c1), pairt(B, g * s2, g * s2, c2)
    k = c1 + c2
    rows = max(n, 128)
    wcat = (torch.randn(rows, 3 * k, device='cuda') * 0.05).to(torch.bfloat16)
    w1 = (torch.randn(rows, 3 * c1, device='cuda') * 0.05).to(torch.bfloat16)
    w2 = (torch.randn(rows, 3 * c2, device='cuda') * 0.05).to(torch.bfloat16)
    bias = torch.randn(n, device='cuda')
    out, sk = pairt(B, g, g, n), pairt(B, g, g, n)
    sign = torch.zeros(B, g, g, n // 8, dtype=torch.uint8, device='cuda')
    mask = torch.randint(0, 256, (B, g, g, n // 8), dtype=torch.uint8, device='cuda')
    kw = dict(batch=B, grid=(g, g), dst_hw=(g, g), taps=[(0, 0)])
    ep = dict(mask_bits=mask) if bwd else dict(bias=bias, sign_out=sign, flags=1)
    # today's two launches: the shortcut on its own, then the 1x1 with the residual
    if bwd:
        da = gemm_pair_desc(a1, w1, out, n, c1, 3 * c1, n, rows, w_lo_off=c1, src_hw=(g, g), k_per_tap=c1, mask_bits=mask, **kw)
        db = gemm_pair_desc(a2, w2, out, n, c2, 3 * c2, n, rows, w_lo_off=c2, src_hw=(g, g), k_per_tap=c2, res=out, mask_bits=mask, **kw)
    else:
        da = gemm_pair_desc(a2, w2, sk, n, c2, 3 * c2, n, rows, w_lo_off=c2, src_hw=(g * s2, g * s2), stride=(s2, s2), k_per_tap=c2, bias=bias, **kw)
        db = gemm_pair_desc(a1, w1, out, n, c1, 3 * c1, n, rows, w_lo_off=c1, src_hw=(g, g), k_per_tap=c1, res=sk, **ep, **kw)
    ta, tb, tab = timeit([da]), timeit([db]), timeit([da, db])
    print('%s  M=%d K=%d+%d N=%d: separate %s + %s us, back to back %s us' % (name, B * g * g, c1, c2, n, ['%.0f' % t for t in ta], ['%.0f' % t for t in tb], ['%.0f' % t for t in tab]), flush=True)
    for tile in ((0, 0), (256, 64), (128, 64), (128, 128), (256, 128), (256, 256), (224, 256), (224, 128)):
        if tile[1] > max(n, 64) and tile != (0, 0):
            continue
        d = gemm_pair_desc(a1, wcat, out, n, c1, 3 * k, n, rows, w_lo_off=k, src_hw=(g, g), k_per_tap=c1, tile=tile,
                           src2=(a2, (g * s2, g * s2), (s2, s2), c2, c2), **ep, **kw)
        t = timeit([d])
        print('    fused tile_m x tile_n = %3d x %3d: %s us' % (tile[0], tile[1], ['%.0f' % x for x in t]), flush=True)
    del a1, a2, out, sk
    torch.cuda.empty_cache()
