"""The instances of k_conv3x3_tail_pair the reference-precision engine launches in layer1 (B = 256, 56 x 56, C = 64, slab staging) with the
1x1 expansion's fragment table loaded from L2 by every wave (tables 0) and staged in LDS once per workgroup (tables 1), back to back: NEXT
(skip pair + the neighbour's reduction), NEXT + XS (the projection shortcut as extra K steps + the neighbour's reduction) and plain (skip
pair only), and XS alone; forward form (biases, ReLU, sign tensors) and backward form (1-bit masks).  us per call, three groups of ten, sorted; measured
twice, alternating; after every instance the outputs of the two modes are compared bit for bit.

    python scratch/time_tail_tables.py [B]"""
import ctypes, sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from robustart_amd import _lib

lib = _lib.load()
sp = _lib.stream_ptr
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
H = W = 56
C, N = 64, 256
P = B * H * W


def pairt(*shape):
    return (torch.randn(2, *shape, device='cuda') * 0.5).to(torch.bfloat16)


def timeit(d, reps=10, groups=3):
    for _ in range(3):
        _lib.check(lib.rart_conv3x3_tail_pair(ctypes.byref(d), sp()))
    torch.cuda.synchronize()
    ts = []
    for _ in range(groups):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            _lib.check(lib.rart_conv3x3_tail_pair(ctypes.byref(d), sp()))
        b.record()
        torch.cuda.synchronize()
        ts.append(round(a.elapsed_time(b) / reps * 1000, 1))
    return sorted(ts)


src, dst, res, dstn, x = pairt(P, C), pairt(P, N), pairt(P, N), pairt(P, C), pairt(P, C)
tab = (torch.randn(C, 3 * 9 * C, device='cuda') * 0.05).to(torch.bfloat16)
tail, ntab, tx = pairt(N * C) * 0.1, pairt(N * C) * 0.1, pairt(N * C) * 0.1
b2, b3, bn = torch.randn(C, device='cuda'), torch.randn(N, device='cuda'), torch.randn(C, device='cuda')
sm, so, sn = (torch.zeros(P, c // 8, dtype=torch.uint8, device='cuda') for c in (C, N, C))
mm, mo, mn = (torch.randint(0, 256, (P, c // 8), dtype=torch.uint8, device='cuda') for c in (C, N, C))


def desc(nxt, xs, backward):
    d = _lib.ConvTailDesc()
    d.a_hi, d.a_lo, d.w_hi, d.w_lo = src[0].data_ptr(), src[1].data_ptr(), tab.data_ptr(), tab.data_ptr() + 2 * 9 * C
    d.t_hi, d.t_lo, d.dst_hi, d.dst_lo = tail[0].data_ptr(), tail[1].data_ptr(), dst[0].data_ptr(), dst[1].data_ptr()
    d.batch, d.h, d.w, d.c_mid, d.ldw = B, H, W, C, 3 * 9 * C
    for i in range(9):
        d.tap_dy[i], d.tap_dx[i] = (1 - i // 3, 1 - i % 3) if backward else (i // 3 - 1, i % 3 - 1)
    if xs:
        d.x_hi, d.x_lo, d.tx_hi, d.tx_lo = x[0].data_ptr(), x[1].data_ptr(), tx[0].data_ptr(), tx[1].data_ptr()
    else:
        d.res_hi, d.res_lo = res[0].data_ptr(), res[1].data_ptr()
    if backward:
        d.mask_mid, d.mask_out = mm.data_ptr(), mo.data_ptr()
    else:
        d.bias_mid, d.bias_out, d.sign_mid, d.sign_out = b2.data_ptr(), b3.data_ptr(), sm.data_ptr(), so.data_ptr()
        d.relu_mid = d.relu_out = 1
    if nxt:
        d.n_hi, d.n_lo, d.dstn_hi, d.dstn_lo = ntab[0].data_ptr(), ntab[1].data_ptr(), dstn[0].data_ptr(), dstn[1].data_ptr()
        if backward:
            d.mask_next = mn.data_ptr()
        else:
            d.bias_next, d.sign_next, d.relu_next = bn.data_ptr(), sn.data_ptr(), 1
    return d


old = lib.rart_conv3x3_tail_pair_get_tables()
assert lib.rart_conv3x3_tail_pair_get_staging() == 1, 'the table buffers exist on the slab path only'
try:
    for name, nxt, xs, backward in (('next_fwd', 1, 0, 0), ('next_bwd', 1, 0, 1), ('next_xs_fwd', 1, 1, 0), ('plain_fwd', 0, 0, 0), ('plain_bwd', 0, 0, 1),
                                    ('xs_fwd', 0, 1, 0)):
        d = desc(nxt, xs, backward)
        r, outs = {}, {}
        for tables in (0, 1, 0, 1):
            _lib.check(lib.rart_conv3x3_tail_pair_set_tables(tables))
            key = ('direct', 'lds')[tables] + ('_again' if ('direct', 'lds')[tables] in r else '')
            dst.zero_(); dstn.zero_(); sm.zero_(); so.zero_(); sn.zero_()
            r[key] = timeit(d)
            outs[tables] = [t.view(torch.int16).clone() if t.dtype == torch.bfloat16 else t.clone() for t in (dst, dstn, sm, so, sn)]
        r['bit_identical'] = bool(all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])))
        print(name, json.dumps(r), flush=True)
finally:
    lib.rart_conv3x3_tail_pair_set_tables(old)
