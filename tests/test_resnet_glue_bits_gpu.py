"""The glue kernels of the ResNet-50 engines and the ViT pixel-gradient scatter, bit for bit against a recording:
rart_engine_maxpool_keep / _maxpool_pair, rart_engine_maxpool_bwd[_pair], rart_engine_avgpool[_bwd][_pair], rart_f32_to_bf16_rows /
rart_f32_to_pair_rows, rart_engine_stem_col2im[_f32] (csrc/engine_aux.hip: one kernel text per operation, instantiated for bf16 and
for pair storage) and rart_vit_unpatchify_f32 / rart_vit_unpatchify_from_f32 (csrc/vit_bwd.hip: one kernel for both patch types).
tests/golden/resnet_glue_bits.json was recorded by tests/golden/make_resnet_glue_bits.py from the commit BEFORE the bf16 and the pair
copies of these kernels were merged (the file names it).  tests/test_stem_glue_kernels_gpu.py and
tests/test_shared_train_kernels_gpu.py hold the same entries to references of their own, several of them only to fp64 bounds; this
file holds them to "same operations, same order, same rounding points, same packer".

Per case the recording has a sha256 of the input bytes and one of every WHOLE output buffer: GUARD elements behind what the call
names and, for a pair, the GAP elements between its planes included, pre-filled with the bf16 NaN 0x7FA5 (fp32 buffers: 0x7FA57FA5,
byte buffers: 0xA5), so a store outside the contract changes the hash as well.  The inputs are rebuilt from seeds; an input hash that
differs fails as "inputs drifted" before any kernel is blamed.  The recording is never remade after a kernel edit: a mismatch means
the code changed the arithmetic, and the fix goes into the code.

Cases (the smallest shapes of the two modules above):
  * max pool forward and backward, both storages, at R.POOL_SHAPES on the relu(randn) inputs with their planted windows; the forward
    with argmax_out / sign_out present and null; the backward on the reference's codes and randn gradients.  Pair planes lie GAP
    elements apart, with NaN between the planes of an input.
  * average pool forward and backward, both storages, at AVG_SHAPES; y holds +0, -0 and negative values (pair: their sign bytes).
  * both row converters at ROW_SHAPES, on the special bit patterns of tests/test_shared_train_kernels_gpu.py.
  * both col2im entries at C2I_SHAPES on randn patches (NaN in columns 147..151), std null and the ImageNet std.
  * both unpatchify entries: 16 x 16 with patch 8 and row stride 192 (bf16 patches), 8 x 8 with patch 4 and row stride 64 (fp32),
    one image and two.
  * what each packer makes of +Inf and NaN, one case per entry that rounds on store: max pool backward at (2, 2, 8, 8) with the two
    planted in dpool under windows whose code is not 15, average pool forward (in x) and backward (in dpool, under y > 0) at
    (1, 1, 8), the row converters at (1, 1, 8) with the one source element +Inf, and again NaN."""
import ctypes
import hashlib
import json
import os

import pytest
import torch

import _stem_glue_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resnet_glue_bits.json')
PRECS = ('bf16', 'pair')
SENT, SENT32, SENT8 = 0x7FA5, 0x7FA57FA5, 0xA5      # a bf16 NaN; the same bytes as an fp32 NaN and as a byte
GUARD = 64                                          # elements behind every output
GAP = 64                                            # elements between the planes of a pair
INF_BITS, NAN_BITS = 0x7F80, 0x7FC0
NAN = float('nan')
AVG_SHAPES = ((1, 1, 8), (3, 49, 2048), (2, 196, 768))
ROW_SHAPES = ((1, 1, 8), (3, 63, 64), (4, 1000, 1024))
C2I_SHAPES = ((1, 16, 32), (2, 32, 64), (1, 48, 32))
NONFINITE_POOL, NONFINITE_AVG, NONFINITE_ROWS = (2, 2, 8, 8), (1, 1, 8), (1, 1, 8)
UNPATCH = {'bf16': (16, 16, 8, 192), 'f32': (8, 8, 4, 64)}          # h, w, patch, row stride


def _cases():
    out = []
    for prec in PRECS:
        out += [('maxpool_fwd', prec) + s + (o,) for s in R.POOL_SHAPES for o in ('arg_sign', 'null')]
        out += [('maxpool_bwd', prec) + s + ('randn',) for s in R.POOL_SHAPES] + [('maxpool_bwd', prec) + NONFINITE_POOL + ('nonfinite',)]
        for op in ('avgpool_fwd', 'avgpool_bwd'):
            out += [(op, prec) + s + ('randn',) for s in AVG_SHAPES] + [(op, prec) + NONFINITE_AVG + ('nonfinite',)]
        out += [('rows', prec) + s + ('special',) for s in ROW_SHAPES] + [('rows', prec) + NONFINITE_ROWS + (k,) for k in ('inf', 'nan')]
    for el in ('bf16', 'f32'):
        out += [('col2im', el) + s + (std,) for s in C2I_SHAPES for std in ('nostd', 'imagenet')]
        out += [('unpatchify', el, n) + UNPATCH[el] for n in (1, 2)]
    return out


def case_id(case):
    return '-'.join(str(f) for f in case)


CASES = _cases()


def _lib():
    from robustart_amd import _lib as L
    return L, L.load()


def sha(tensors):
    """sha256 over the bytes of the tensors, in order (None: skipped)"""
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _bits(t):
    return t.view(torch.int16)


def _seed(*fields):
    s = 0
    for f in fields:
        s = s * 1009 + int(f)
    return 700000 + s % 1000003


def _sentinel(numel, dtype=torch.bfloat16):
    """an output buffer of numel + GUARD elements, all of them the sentinel"""
    if dtype == torch.uint8:
        return torch.full((numel + GUARD,), SENT8, dtype=torch.uint8, device='cuda')
    if dtype == torch.float32:
        return torch.full((numel + GUARD,), SENT32, dtype=torch.int32, device='cuda').view(torch.float32)
    return torch.full((numel + GUARD,), SENT, dtype=torch.int16, device='cuda').view(torch.bfloat16)


def _pair_sentinel(numel):
    """[hi | GAP | lo | GUARD], all of it the sentinel -> the buffer and lo_off"""
    return _sentinel(2 * numel + GAP), numel + GAP


def _store(v, prec):
    """fp32 values on the CPU -> the device operand and its lo_off (bf16: None): bf16, or [hi | GAP of NaN | lo]"""
    if prec == 'bf16':
        return v.to(torch.bfloat16).reshape(-1).cuda(), None
    hi, lo = R.split(v.float())
    buf = torch.full((2 * v.numel() + GAP,), NAN, dtype=torch.bfloat16)
    buf[:v.numel()] = hi.reshape(-1)
    buf[v.numel() + GAP:] = lo.reshape(-1)
    return buf.cuda(), v.numel() + GAP


def _plant(buf, lo_off, at, bits):
    """element `at` of a stored operand becomes `bits` (a pair: in the hi plane, +0 in the lo plane)"""
    _bits(buf)[at] = bits
    if lo_off is not None:
        _bits(buf)[at + lo_off] = 0


def _out(numel, prec):
    return (_sentinel(numel), None) if prec == 'bf16' else _pair_sentinel(numel)


def _c3(std):
    return (ctypes.c_float * 3)(*R.IMAGENET_STD) if std == 'imagenet' else None


# ------------------------------------------------------------------ max pool
def _pool_input(prec, shape):
    """-> the NCHW case on the CPU (fp64 for bf16, fp32 canonical pair values) and its stored NHWC operand"""
    x = R.pool_case('relu' if prec == 'bf16' else 'relu_pair', shape)
    return x, _store(R.nhwc(x), prec)


def _run_maxpool_fwd(prec, n, h, w, c, outs):
    L, lib = _lib()
    _, (xd, x_lo) = _pool_input(prec, (n, h, w, c))
    items = n * (h // 2) * (w // 2) * c
    arg = _sentinel(items, torch.uint8) if outs == 'arg_sign' else None
    sign = _sentinel(items // 8, torch.uint8) if outs == 'arg_sign' else None
    out, out_lo = _out(items, prec)
    if prec == 'bf16':
        L.check(lib.rart_engine_maxpool_keep(L.ptr(xd), L.ptr(out), L.ptr(arg), L.ptr(sign), n, h, w, c, L.stream_ptr()))
    else:
        L.check(lib.rart_engine_maxpool_pair(L.ptr(xd), x_lo, L.ptr(out), out_lo, L.ptr(arg), L.ptr(sign), n, h, w, c, L.stream_ptr()))
    res = dict(out=out)
    if outs == 'arg_sign':
        res.update(arg=arg, sign=sign)
    return [xd], res


def _run_maxpool_bwd(prec, n, h, w, c, kind):
    L, lib = _lib()
    x, (xd, _) = _pool_input(prec, (n, h, w, c))
    codes = R.nhwc(R.maxpool_ref(x.double())[1]).reshape(-1)
    g = torch.randn(n, h // 2, w // 2, c, generator=torch.Generator().manual_seed(_seed(1, n, h, w, c)))
    dp, dp_lo = _store(g, prec)
    if kind == 'nonfinite':
        live = (codes != 15).nonzero().view(-1)
        _plant(dp, dp_lo, int(live[0]), INF_BITS)
        _plant(dp, dp_lo, int(live[len(live) // 2]), NAN_BITS)
    codes = codes.cuda()
    dz, dz_lo = _out(n * h * w * c, prec)
    if prec == 'bf16':
        L.check(lib.rart_engine_maxpool_bwd(L.ptr(xd), L.ptr(codes), L.ptr(dp), L.ptr(dz), n, h, w, c, L.stream_ptr()))
        return [xd, codes, dp], dict(dz=dz)
    L.check(lib.rart_engine_maxpool_bwd_pair(L.ptr(codes), L.ptr(dp), dp_lo, L.ptr(dz), dz_lo, n, h, w, c, L.stream_ptr()))
    return [codes, dp], dict(dz=dz)


# ------------------------------------------------------------------ global average pool
def _run_avgpool_fwd(prec, n, hw, c, kind):
    L, lib = _lib()
    x, x_lo = _store(torch.randn(n, hw, c, generator=torch.Generator().manual_seed(_seed(2, n, hw, c))), prec)
    if kind == 'nonfinite':
        _plant(x, x_lo, 3, INF_BITS)
        _plant(x, x_lo, 5, NAN_BITS)
    out, out_lo = _out(n * c, prec)
    if prec == 'bf16':
        L.check(lib.rart_engine_avgpool(L.ptr(x), L.ptr(out), n, hw, c, L.stream_ptr()))
    else:
        L.check(lib.rart_engine_avgpool_pair(L.ptr(x), x_lo, L.ptr(out), out_lo, n, hw, c, L.stream_ptr()))
    return [x], dict(out=out)


def _run_avgpool_bwd(prec, n, hw, c, kind):
    L, lib = _lib()
    g = torch.Generator().manual_seed(_seed(3, n, hw, c))
    y = torch.randn(n, hw, c, generator=g)
    y.view(-1)[0::7] = 0.0
    y.view(-1)[1::7] = -0.0
    y.view(-1)[2::7] = -1.5
    dp, dp_lo = _store(torch.randn(n, c, generator=g), prec)
    if kind == 'nonfinite':
        y.view(-1)[3], y.view(-1)[5] = 1.0, 2.0
        _plant(dp, dp_lo, 3, INF_BITS)
        _plant(dp, dp_lo, 5, NAN_BITS)
    dz, dz_lo = _out(n * hw * c, prec)
    if prec == 'bf16':
        yd = y.to(torch.bfloat16).cuda()
        L.check(lib.rart_engine_avgpool_bwd(L.ptr(yd), L.ptr(dp), L.ptr(dz), n, hw, c, L.stream_ptr()))
        return [yd, dp], dict(dz=dz)
    sign = ((y > 0).view(n, hw, c // 8, 8).int() * (2 ** torch.arange(8, dtype=torch.int32))).sum(-1).to(torch.uint8).cuda()
    L.check(lib.rart_engine_avgpool_bwd_pair(L.ptr(sign), L.ptr(dp), dp_lo, L.ptr(dz), dz_lo, n, hw, c, L.stream_ptr()))
    return [sign, dp], dict(dz=dz)


# ------------------------------------------------------------------ fp32 rows -> bf16 / pair rows
def _run_rows(prec, rows, cols, dst_cols, kind):
    L, lib = _lib()
    from test_shared_train_kernels_gpu import _rows_src
    src = _rows_src(rows, cols)
    if kind != 'special':
        src[0, 0] = float(kind)
    src = src.cuda()
    dst, dst_lo = _out(rows * dst_cols, prec)
    if prec == 'bf16':
        L.check(lib.rart_f32_to_bf16_rows(L.ptr(src), L.ptr(dst), rows, cols, dst_cols, L.stream_ptr()))
    else:
        L.check(lib.rart_f32_to_pair_rows(L.ptr(src), L.ptr(dst), dst_lo, rows, cols, dst_cols, L.stream_ptr()))
    return [src], dict(dst=dst)


# ------------------------------------------------------------------ col2im, unpatchify
def _run_col2im(el, n, h, w, std):
    L, lib = _lib()
    dtype = torch.float32 if el == 'f32' else torch.bfloat16
    patches = torch.full((n, h // 2, w // 2, R.PATCH_COLS), NAN, dtype=dtype)
    patches[..., :147] = torch.randn(n, h // 2, w // 2, 147, generator=torch.Generator().manual_seed(_seed(4, n, h, w))).to(dtype)
    patches = patches.cuda()
    grad = _sentinel(n * 3 * h * w, torch.float32)
    fn = lib.rart_engine_stem_col2im_f32 if el == 'f32' else lib.rart_engine_stem_col2im
    L.check(fn(L.ptr(patches), L.ptr(grad), n, h, w, R.PATCH_COLS, _c3(std), L.stream_ptr()))
    return [patches], dict(grad=grad)


def _run_unpatchify(el, n, h, w, ps, ld):
    L, lib = _lib()
    dtype = torch.float32 if el == 'f32' else torch.bfloat16
    dp = torch.randn(n * (h // ps) * (w // ps), ld, generator=torch.Generator().manual_seed(_seed(5, n, h, w, ps))).to(dtype).cuda()
    grad = _sentinel(n * 3 * h * w, torch.float32)
    fn = lib.rart_vit_unpatchify_from_f32 if el == 'f32' else lib.rart_vit_unpatchify_f32
    L.check(fn(L.ptr(dp), L.ptr(grad), n, h, w, ps, ld, _c3('imagenet'), L.stream_ptr()))
    return [dp], dict(grad=grad)


RUNNERS = dict(maxpool_fwd=_run_maxpool_fwd, maxpool_bwd=_run_maxpool_bwd, avgpool_fwd=_run_avgpool_fwd, avgpool_bwd=_run_avgpool_bwd,
               rows=_run_rows, col2im=_run_col2im, unpatchify=_run_unpatchify)


def run_case(case):
    """-> the recording's entry for the case: {'inputs': sha256, 'outputs': {buffer: sha256}}"""
    inputs, outputs = RUNNERS[case[0]](*case[1:])
    return {'inputs': sha(inputs), 'outputs': {k: sha([v]) for k, v in outputs.items()}}


_golden = {}


def golden():
    if not _golden:
        with open(GOLDEN) as f:
            _golden.update(json.load(f))
    return _golden


def test_every_case_is_recorded():
    assert sorted(golden()['cases']) == sorted(case_id(c) for c in CASES)


@pytest.mark.parametrize('case', CASES, ids=[case_id(c) for c in CASES])
def test_bits_match_the_recording(case):
    want = golden()['cases'][case_id(case)]
    got = run_case(case)
    assert got['inputs'] == want['inputs'], 'inputs drifted: the operands rebuilt from the seeds are not the recorded ones'
    assert got['outputs'] == want['outputs'], 'output bits differ from the recording (commit %s)' % golden()['commit']
