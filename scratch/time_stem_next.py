"""Stem fold at B = 256: stem forward + layer1.0 conv1 as two launches against the one NEXT launch."""
import ctypes, sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from robustart_amd import _lib
from robustart_amd.model.engine_base import stem_rows, gemm_pair_desc
lib = _lib.load()
B, H, W = 256, 224, 224
g = torch.Generator().manual_seed(5)
def split(t):
    hi = t.to(torch.bfloat16); return torch.stack([hi, (t - hi.float()).to(torch.bfloat16)]).contiguous()
wf = split(stem_rows(torch.randn(64, 3, 7, 7, generator=g) * 0.1)).cuda()
bias = torch.randn(64, generator=g).cuda()
w1 = split(torch.randn(64, 64, generator=g) * 0.125).cuda()
tab = torch.cat([w1[0], w1[1], w1[0]], 1).contiguous()
b1 = torch.randn(64, generator=g).cuda()
xf = torch.rand(B, 3, H, W, generator=g).cuda()
xu = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
h2, w2 = H // 4, W // 4
p1 = torch.empty(2, B, h2, w2, 64, dtype=torch.bfloat16, device='cuda')
ya = torch.empty(2, B, h2, w2, 64, dtype=torch.bfloat16, device='cuda')
arg = torch.empty(B, h2, w2, 64, dtype=torch.uint8, device='cuda')
sign = torch.empty(B, h2, w2, 8, dtype=torch.uint8, device='cuda')
sa = torch.empty(B, h2, w2, 8, dtype=torch.uint8, device='cuda')
m3 = (ctypes.c_float * 3)(0.485, 0.456, 0.406); s3 = (ctypes.c_float * 3)(0.229, 0.224, 0.225)
sp = _lib.stream_ptr()
P = _lib.ptr
d = gemm_pair_desc(p1, tab, ya, 64, 64, 192, 64, 64, bias=b1, sign_out=sa, flags=1, w_lo_off=64, batch=B, grid=(h2, w2), src_hw=(h2, w2),
                   k_per_tap=64, taps=[(0, 0)], dst_hw=(h2, w2))
def stem(x, u8): _lib.check(lib.rart_engine_stem_fwd_fused_pair(P(x), u8, P(wf[0]), P(wf[1]), P(bias), P(p1[0]), P(p1[1]), P(arg), P(sign), B, H, W, m3, s3, sp))
def conv1(): _lib.check(lib.rart_gemm_pair_bf16(ctypes.byref(d), sp))
def nxt(x, u8): _lib.check(lib.rart_engine_stem_fwd_next_pair(P(x), u8, P(wf[0]), P(wf[1]), P(bias), P(p1[0]), P(p1[1]), P(arg), P(sign),
                ctypes.c_void_p(tab.data_ptr()), ctypes.c_void_p(tab.data_ptr() + 128), 192, P(b1), P(ya[0]), P(ya[1]), P(sa), B, H, W, m3, s3, sp))
def t(fn, n=20, groups=3):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(groups):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): fn()
        e1.record(); torch.cuda.synchronize()
        out.append(round(e0.elapsed_time(e1) / n * 1e3, 1))
    return sorted(out)
res = {}
for name, x, u8 in (('f32', xf, 0), ('u8', xu, 1)):
    res[name] = {'stem': t(lambda: stem(x, u8)), 'conv1': t(conv1), 'stem_then_conv1': t(lambda: (stem(x, u8), conv1())), 'stem_next': t(lambda: nxt(x, u8))}
    print(name, json.dumps(res[name]), flush=True)
