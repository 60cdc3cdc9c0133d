"""The class launches of the stride-2 first blocks at B = 256 against the launches they replace, back to back, per layer: the four
parity-class launches of the 3x3 backward (3x3_*), and conv1^T + shortcut^T against conv1^T per parity with the shortcut^T as the second
source of the class (0, 0) (sc_*); every forced tile form beside the automatic one.  us per call, three groups of ten, sorted.

    python scratch/time_class_launch.py [layer2 layer3 layer4]"""
import ctypes, sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from robustart_amd import _lib
from robustart_amd.model.engine_base import gemm_pair_desc, gemm_pair_cls_desc, conv_tap_classes

lib = _lib.load()
sp = _lib.stream_ptr


def pairt(*shape):
    return (torch.randn(2, *shape, device='cuda') * 0.5).to(torch.bfloat16)


def launch(d):
    if isinstance(d, _lib.GemmPairClsDesc):
        _lib.check(lib.rart_gemm_pair_classes_bf16(ctypes.byref(d), sp()))
    elif isinstance(d, _lib.GemmPair2Desc):
        _lib.check(lib.rart_gemm_pair2_bf16(ctypes.byref(d), sp()))
    else:
        _lib.check(lib.rart_gemm_pair_bf16(ctypes.byref(d), sp()))


def timeit(descs, reps=10, groups=3):
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
        ts.append(round(a.elapsed_time(b) / reps * 1000, 1))
    return sorted(ts)


B = 256
PAR = ((0, 0), (0, 1), (1, 0), (1, 1))
res = {}
only = sys.argv[1:]
for name, g, c, cin, dsout in (('layer2', 28, 128, 256, 512), ('layer3', 14, 256, 512, 1024), ('layer4', 7, 512, 1024, 2048)):
    if only and name not in only:
        continue
    # ---- the stride-2 3x3 backward: dzb [B][g][g][c] -> dza [B][2g][2g][c]
    cls = conv_tap_classes(3, 3, 2, 1)[2]
    dzb, dza = pairt(B, g, g, c), pairt(B, 2 * g, 2 * g, c)
    mask = torch.randint(0, 256, (B, 2 * g, 2 * g, c // 8), dtype=torch.uint8, device='cuda')
    rows = max(c, 128)
    ks = [c * len(t) for _, t, _ in cls]
    offs = [sum(ks[:i]) for i in range(4)]
    kt = sum(ks)
    tab = (torch.randn(rows, 3 * kt, device='cuda') * 0.05).to(torch.bfloat16)
    tabs = [(torch.randn(rows, 3 * k, device='cuda') * 0.05).to(torch.bfloat16) for k in ks]
    kw = dict(batch=B, grid=(g, g), src_hw=(g, g), k_per_tap=c, dst_hw=(2 * g, 2 * g), dst_stride=(2, 2), mask_bits=mask)
    sep = [gemm_pair_desc(dzb, tabs[i], dza, c, c, 3 * ks[i], c, rows, w_lo_off=ks[i], taps=cls[i][1], dst_org=cls[i][0], **kw) for i in range(4)]
    one = gemm_pair_cls_desc(dzb, tab, dza, c, c, 3 * kt, c, rows, [(cls[i][1], offs[i], cls[i][0], False) for i in range(4)], w_lo_off=kt, **kw)
    r = {'3x3_separate': timeit(sep), '3x3_class': timeit([one])}
    for tile in ((256, 256), (224, 256), (256, 128), (128, 128), (256, 64)):
        if tile[1] > max(c, 64):
            continue
        t1 = gemm_pair_cls_desc(dzb, tab, dza, c, c, 3 * kt, c, rows, [(cls[i][1], offs[i], cls[i][0], False) for i in range(4)], w_lo_off=kt,
                                tile=tile, **kw)
        r['3x3_class_%dx%d' % tile] = timeit([t1])
    print(name, json.dumps(r), flush=True)
    res[name] = r
    # ---- conv1^T + shortcut^T: dza [B][2g][2g][c], dz [B][g][g][dsout] -> dx [B][2g][2g][cin]
    dz, dx = pairt(B, g, g, dsout), pairt(B, 2 * g, 2 * g, cin)
    maskx = torch.randint(0, 256, (B, 2 * g, 2 * g, cin // 8), dtype=torch.uint8, device='cuda')
    w1 = (torch.randn(cin, 3 * c, device='cuda') * 0.05).to(torch.bfloat16)
    wd = (torch.randn(cin, 3 * dsout, device='cuda') * 0.05).to(torch.bfloat16)
    kt = 4 * c + dsout
    tab = (torch.randn(cin, 3 * kt, device='cuda') * 0.05).to(torch.bfloat16)
    offs = [0, c + dsout, 2 * c + dsout, 3 * c + dsout]
    d1 = gemm_pair_desc(dza, w1, dx, cin, c, 3 * c, cin, cin, w_lo_off=c, batch=B, grid=(2 * g, 2 * g), src_hw=(2 * g, 2 * g), k_per_tap=c,
                        taps=[(0, 0)], dst_hw=(2 * g, 2 * g), mask_bits=maskx)
    d2 = gemm_pair_desc(dz, wd, dx, cin, dsout, 3 * dsout, cin, cin, w_lo_off=dsout, batch=B, grid=(g, g), src_hw=(g, g), k_per_tap=dsout,
                        taps=[(0, 0)], dst_hw=(2 * g, 2 * g), dst_stride=(2, 2), res=dx, mask_bits=maskx)
    ckw = dict(w_lo_off=kt, batch=B, grid=(g, g), src_hw=(2 * g, 2 * g), stride=(2, 2), k_per_tap=c, dst_hw=(2 * g, 2 * g), dst_stride=(2, 2),
               mask_bits=maskx, src2=(dz, (g, g), (1, 1), dsout, dsout))
    mk = lambda tile=(0, 0): gemm_pair_cls_desc(dza, tab, dx, cin, c, 3 * kt, cin, cin, [([p], offs[i], p, i == 0) for i, p in enumerate(PAR)],  # noqa: E731
                                                tile=tile, **ckw)
    r = {'sc_conv1T': timeit([d1]), 'sc_shortcutT': timeit([d2]), 'sc_separate': timeit([d1, d2]), 'sc_class': timeit([mk()])}
    for tile in ((256, 256), (224, 256), (256, 128), (256, 64)):
        r['sc_class_%dx%d' % tile] = timeit([mk(tile)])
    print(name, json.dumps(r), flush=True)
    res[name].update(r)
    del dzb, dza, dz, dx
    torch.cuda.empty_cache()
