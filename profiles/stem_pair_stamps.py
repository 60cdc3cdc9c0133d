"""Phase stamps of the two fused pair stem kernels at B = 256, 224 x 224 from a -DRART_STEM_STAMPS lab build:

    python profiles/stem_pair_lab_build.py /tmp/stamps.so -DRART_STEM_STAMPS && python profiles/stem_pair_stamps.py /tmp/stamps.so
Prints one JSON line: s_memtime ticks per phase summed over the waves of five launches (csrc/stem_pair.hip names the entries)."""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robustart_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
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

lib.rart_debug_stem_stamps.restype = ctypes.c_int
lib.rart_debug_stem_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
buf = (ctypes.c_ulonglong * 16)()
def stamps(fn, n=5):
    for _ in range(3): fn()
    torch.cuda.synchronize(); assert lib.rart_debug_stem_stamps(buf, 1) == 0
    for _ in range(n): fn()
    torch.cuda.synchronize(); assert lib.rart_debug_stem_stamps(buf, 1) == 0
    return [int(v) for v in buf]
out = {'lib': os.path.basename(sys.argv[1]), 'unit': 's_memtime ticks summed over waves; last entries = counts',
       'fwd_names': ['stage(wait+convert+write)', 'mma(+next loads issue)', 'barrier after mma', 'relu+store tile', 'pool+global store', 'tiles*waves', 'whole loop', 'waves'],
       'bwd_names': ['stage', 'pool backward', 'weights+mma', 'epilogue', 'whole kernel', 'waves']}
v = stamps(lambda: fwd(xf, 0)); out['fwd_f32'] = v[8:16]
v = stamps(lambda: fwd(xu, 1)); out['fwd_u8'] = v[8:16]
v = stamps(bwd); out['bwd'] = v[0:6]
print(json.dumps(out), flush=True)
