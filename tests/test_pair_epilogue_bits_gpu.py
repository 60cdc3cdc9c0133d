"""The epilogues of the split-bf16 pair kernels, bit for bit against a recording: gp_epilogue (csrc/rart_gemm_pair_dev.h) under
k_gemm_pair and k_gemm_pair_pp (csrc/gemm_pair.hip, csrc/gemm_pair_pp.hip), and the 1x1 chunk loop of k_conv3x3_tail_pair
(csrc/conv_tail_pair.hip).  tests/golden/pair_epilogue_bits.json was recorded by tests/golden/make_pair_epilogue_bits.py from the commit
BEFORE gp_epilogue was given its counted vmcnt wait per block, its straight-line operand loads and the conv instances without the GELU
forms (the file names it): where a wave waits and how it requests its operands changes no arithmetic, so every output bit must stay;
the tail kernel's cases hold the same for any later edit of its chunk loop.  Every GEMM case also asks rart_gemm_pair_plan_bf16 what its
descriptor launches and asserts the kernel family and the tile the case is named after.  The scheme is the one of
tests/test_resnet_glue_bits_gpu.py: per case a sha256 of the input bytes and one of every WHOLE output buffer (hi | GAP | lo | GUARD of a pair, sign bytes, the kept pre-activation pair, fp32), pre-filled
with the sentinel, so a store outside the contract changes the hash as well.  The recording is never remade after a kernel edit.

GEMM cases: two images of 14 x 14 -> M = 392 rows: a 256-row tile followed by a ragged one, 224-row tiles by a 168-row one, 128-row
tiles by an 8-row one; K = 64 (two K steps); N = 256, 128 or 72 (72: a column tile whose last seven 8-column segments lie past N).
Every case is forced onto a tile form with tile_m / tile_n: ping-pong 256 x 256, ping-pong 224-row, ping-pong 256 x 128, two-stage
128 x 128, 256 x 64 and 128 x 64.
  * conv1x1 (conv mode, one tap): plain, residual, 1-bit mask, residual + mask, bias + ReLU + sign bytes, fp32 output, and the residual
    + mask and the sign-byte paths once more with the non-temporal streams off (RART_PAIR_NT_MIN_MB).
  * conv3x3: nine taps of 32 channels (K = 9 x 32), pad 1, bias + ReLU + sign bytes.
  * two_source: rart_gemm_pair2_bf16, K1 = 64 + k2 = 64, residual + mask.
  * classes: rart_gemm_pair_classes_bf16, the four parity classes of a stride-2 destination (28 x 28), 1-bit mask.
  * plain: plain products with rows re-based per image on both sides (196 of 197 rows, offset 1): residual + bias, and the three GELU
    forms (GELU, GELU with the pre-activation kept in aux, GELU' of aux).
Tail cases: k_conv3x3_tail_pair at two images of 56 x 56, C = 64: NEXT, NEXT + XS and plain, forward form (biases, ReLU, sign bytes) and
backward form (1-bit masks).
Edge values: the A operand has a row of zeros, a row of +Inf and a row of NaN; residuals hold zeros, negative values, +Inf and NaN."""
import ctypes
import functools
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pair_epilogue_bits.json')
SENT, SENT32, SENT8 = 0x7FA5, 0x7FA57FA5, 0xA5      # a bf16 NaN; the same bytes as an fp32 NaN and as a byte
GUARD, GAP = 64, 64                                 # elements behind every output; between the planes of a pair
B, G, K = 2, 14, 64
M = B * G * G
RELU, OUT_F32, GELU, GELU_BWD, GELU_KEEP = 1, 2, 4, 8, 64
TILES = {'pp256x256': (256, 256), 'pp224x256': (224, 256), 'pp256x128': (256, 128), 'ts128x128': (128, 128), 'ts256x64': (256, 64),
         'ts128x64': (128, 64)}
TILE_N = {'pp256x256': (256, 72), 'pp224x256': (256, 72), 'pp256x128': (128, 72), 'ts128x128': (128, 72), 'ts256x64': (72,), 'ts128x64': (72,)}
CONV_PATHS = ('plain', 'res', 'mask', 'res_mask', 'relu_sign', 'f32', 'res_mask_ntoff', 'relu_sign_ntoff')
PLAIN_PATHS = ('res', 'gelu', 'gelu_keep', 'gelu_bwd')
TAIL = (('next', 'fwd'), ('next', 'bwd'), ('next_xs', 'fwd'), ('next_xs', 'bwd'), ('plain', 'fwd'), ('plain', 'bwd'))


def _cases():
    out = [('conv1x1', p, t, n) for t in TILES for n in TILE_N[t] for p in CONV_PATHS]
    out += [('conv3x3', 'relu_sign', t, n) for t, n in (('pp256x256', 256), ('ts128x128', 128))]
    out += [('two_source', 'res_mask', t, n) for t, n in (('pp256x256', 256), ('pp224x256', 256), ('ts128x64', 72))]
    out += [('classes', 'mask', t, n) for t, n in (('pp256x256', 256), ('pp224x256', 256), ('ts128x64', 72))]
    out += [('plain', p, t, TILE_N[t][0]) for t in TILES for p in PLAIN_PATHS]
    out += [('tail',) + t for t in TAIL]
    return out


def case_id(case):
    return '-'.join(str(f) for f in case)


CASES = _cases()


def _lib():
    from robustart_amd import _lib as L
    return L, L.load()


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _sentinel(numel, dtype=torch.bfloat16):
    """an output buffer of numel + GUARD elements, all of them the sentinel"""
    if dtype == torch.uint8:
        return torch.full((numel + GUARD,), SENT8, dtype=torch.uint8, device='cuda')
    if dtype == torch.float32:
        return torch.full((numel + GUARD,), SENT32, dtype=torch.int32, device='cuda').view(torch.float32)
    return torch.full((numel + GUARD,), SENT, dtype=torch.int16, device='cuda').view(torch.bfloat16)


def _pair_out(numel):
    """[hi | GAP | lo | GUARD], all of it the sentinel -> the buffer, the addresses of its planes"""
    buf = _sentinel(2 * numel + GAP)
    return buf, buf.data_ptr(), buf.data_ptr() + 2 * (numel + GAP)


def _gen(*fields):
    s = 0
    for f in fields:
        s = s * 1009 + sum(ord(c) for c in str(f))
    return torch.Generator().manual_seed(810000 + s % 1000003)


def _split(t):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


def _activations(g, rows, cols):
    """a pair [2][rows][cols] with a row of zeros (3), of +Inf (5) and of NaN (9)"""
    p = _split(torch.randn(rows, cols, generator=g))
    p[:, 3] = 0
    p[0, 5], p[1, 5] = float('inf'), 0
    p[0, 9], p[1, 9] = float('nan'), 0
    return p.cuda()


def _residual(g, numel):
    """a pair [2][numel]: randn (negative values included) with zeros, +Inf and NaN planted"""
    v = torch.randn(numel, generator=g)
    v[0::11] = 0.0
    p = _split(v)
    p[0, 17], p[1, 17] = float('inf'), 0
    p[0, 29], p[1, 29] = float('nan'), 0
    return p.cuda()


def _table(g, n, k):
    """weights [n][k] as rows [hi | lo] (ldw = 2 k, the lo plane k elements behind the hi plane)"""
    w = _split(torch.randn(n, k, generator=g) * 0.08)
    return torch.cat([w[0], w[1]], 1).contiguous().cuda()


class _NtOff:
    """the epilogue's streams as ordinary accesses for the calls inside (the library reads the variable on every call)"""

    def __init__(self, off):
        self.off = off

    def __enter__(self):
        self.old = os.environ.get('RART_PAIR_NT_MIN_MB')
        if self.off:
            os.environ['RART_PAIR_NT_MIN_MB'] = '1000000'

    def __exit__(self, *exc):
        if self.off:
            if self.old is None:
                del os.environ['RART_PAIR_NT_MIN_MB']
            else:
                os.environ['RART_PAIR_NT_MIN_MB'] = self.old


# ------------------------------------------------------------------ the GEMM entries
def _fill_common(d, a, tab, k, n, tile):
    d.a_hi, d.a_lo = a[0].data_ptr(), a[1].data_ptr()
    d.w_hi, d.w_lo = tab.data_ptr(), tab.data_ptr() + 2 * k
    d.N, d.ldw, d.ldc, d.w_rows = n, 2 * k, n, n
    d.tile_m, d.tile_n = TILES[tile]


def _assert_plan(L, lib, d, tile):
    """the descriptor (plain, two-source or class form) launches the kernel family and the tile the case is named after"""
    c = d if isinstance(d, L.GemmPairClsDesc) else L.GemmPairClsDesc()
    if c is not d:
        ctypes.memmove(ctypes.byref(c), ctypes.byref(d), ctypes.sizeof(d))      # (`one` / `two` lead the class descriptor)
    plan = L.GemmPairPlan()
    L.check(lib.rart_gemm_pair_plan_bf16(ctypes.byref(c), 256, ctypes.byref(plan)))
    r = plan.launch[0]
    tm, tn = TILES[tile]
    want = (1, 1, 256, tn, tm if tm == 224 else 256) if tile.startswith('pp') else (1, 0, tm, tn, tm)
    assert (plan.n_launches, r.family, r.tile_m, r.tile_n, r.tile_rows) == want, (tile, r.family, r.tile_m, r.tile_n, r.tile_rows)


def _epilogue_operands(d, g, path, numel, n, keep):
    """the outputs and epilogue operands a path names -> (inputs, outputs)"""
    ins, outs = [], {}
    base = path.replace('_ntoff', '')
    if base == 'f32':
        out = _sentinel(numel, torch.float32)
        d.dst_hi, d.flags = out.data_ptr(), d.flags | OUT_F32
        outs['f32'] = out
    else:
        out, d.dst_hi, d.dst_lo = _pair_out(numel)
        outs['pair'] = out
    if base in ('res', 'res_mask'):
        res = _residual(g, numel)
        d.res_hi, d.res_lo = res[0].data_ptr(), res[1].data_ptr()
        ins.append(res)
    if base in ('mask', 'res_mask'):
        mask = torch.randint(0, 256, (numel // 8,), generator=g, dtype=torch.uint8).cuda()
        d.mask_bits = mask.data_ptr()
        ins.append(mask)
    if base == 'relu_sign':
        bias = torch.randn(n, generator=g).cuda()
        sign = _sentinel(numel // 8, torch.uint8)
        d.bias, d.sign_out, d.flags = bias.data_ptr(), sign.data_ptr(), d.flags | RELU
        ins.append(bias)
        outs['sign'] = sign
    keep += ins + list(outs.values())
    return ins, outs


def _run_conv(kind, path, tile, n):
    L, lib = _lib()
    g = _gen(kind, path, tile, n)
    keep = []
    if kind == 'classes':
        d = L.GemmPairClsDesc()
        one = d.two.one
    elif kind == 'two_source':
        d = L.GemmPair2Desc()
        one = d.one
    else:
        d = one = L.GemmPairDesc()
    c, taps, src, stride, dst = K, [(0, 0)], G, 1, G
    if kind == 'conv3x3':
        c, taps = 32, [(i // 3 - 1, i % 3 - 1) for i in range(9)]
    if kind == 'classes':
        taps, src, stride, dst = [(0, 0), (0, 1), (1, 0), (1, 1)], 2 * G, 2, 2 * G
    ktab = c * len(taps) + (K if kind == 'two_source' else 0)
    a = _activations(g, B * src * src, c)
    tab = _table(g, n, ktab)
    _fill_common(one, a, tab, ktab, n, tile)
    one.lda = c
    one.conv, one.batch, one.grid_h, one.grid_w, one.src_h, one.src_w, one.sy, one.sx = 1, B, G, G, src, src, stride, stride
    one.k_per_tap, one.n_taps = c, len(taps)
    for i, (dy, dx) in enumerate(taps):
        one.tap_dy[i], one.tap_dx[i] = dy, dx
    one.dst_h, one.dst_w, one.dst_sy, one.dst_sx = dst, dst, stride, stride
    ins, outs = _epilogue_operands(one, g, path, B * dst * dst * n, n, keep)
    ins += [a, tab]
    with _NtOff(path.endswith('_ntoff')):
        if kind == 'classes':
            d.n_classes = 4
            for i, (oy, ox) in enumerate(taps):
                k = d.cls[i]
                k.tap_begin, k.n_taps, k.k_off, k.dst_oy, k.dst_ox, k.src2 = i, 1, c * i, oy, ox, 0
            _assert_plan(L, lib, d, tile)
            L.check(lib.rart_gemm_pair_classes_bf16(ctypes.byref(d), L.stream_ptr()))
        elif kind == 'two_source':
            a2 = _activations(g, M, K)
            d.a2_hi, d.a2_lo = a2[0].data_ptr(), a2[1].data_ptr()
            d.lda2, d.k2, d.src2_h, d.src2_w, d.sy2, d.sx2 = K, K, G, G, 1, 1
            ins.append(a2)
            _assert_plan(L, lib, d, tile)
            L.check(lib.rart_gemm_pair2_bf16(ctypes.byref(d), L.stream_ptr()))
        else:
            _assert_plan(L, lib, d, tile)
            L.check(lib.rart_gemm_pair_bf16(ctypes.byref(d), L.stream_ptr()))
    torch.cuda.synchronize()
    return ins, outs


def _run_plain(path, tile, n):
    """392 rows = two images of 196; source and destination rows re-based to 197 per image, offset 1 (ViT's class-token slot)"""
    L, lib = _lib()
    g = _gen('plain', path, tile, n)
    rows = 2 * 197
    d = L.GemmPairDesc()
    a = _activations(g, rows, K)
    tab = _table(g, n, K)
    _fill_common(d, a, tab, K, n, tile)
    d.M, d.K, d.lda = M, K, K
    d.rows_per_image, d.src_rows_per_image, d.src_row_off, d.dst_rows_per_image, d.dst_row_off = 196, 197, 1, 197, 1
    bias = torch.randn(n, generator=g).cuda()
    d.bias = bias.data_ptr()
    ins, outs = [a, tab, bias], {}
    out, d.dst_hi, d.dst_lo = _pair_out(rows * n)
    outs['pair'] = out
    if path == 'res':
        res = _residual(g, rows * n)
        d.res_hi, d.res_lo = res[0].data_ptr(), res[1].data_ptr()
        ins.append(res)
    elif path == 'gelu':
        d.flags = GELU
    elif path == 'gelu_keep':
        aux, d.aux_hi, d.aux_lo = _pair_out(rows * n)
        d.flags = GELU_KEEP
        outs['aux'] = aux
    elif path == 'gelu_bwd':
        aux = _residual(g, rows * n)
        d.aux_hi, d.aux_lo, d.flags = aux[0].data_ptr(), aux[1].data_ptr(), GELU_BWD
        ins.append(aux)
    _assert_plan(L, lib, d, tile)
    L.check(lib.rart_gemm_pair_bf16(ctypes.byref(d), L.stream_ptr()))
    torch.cuda.synchronize()
    return ins, outs


# ------------------------------------------------------------------ the layer1 tail kernel
TB, TH, TC, TN = 2, 56, 64, 256
TP = TB * TH * TH


@functools.lru_cache(maxsize=None)
def _tail_operands():
    """made once and left unchanged: the input pairs, the 3x3 table [hi | lo | hi], the fragment tables, biases and masks"""
    g = _gen('tail')
    src, x = _activations(g, TP, TC), _activations(g, TP, TC)
    res = _residual(g, TP * TN)
    w = _split(torch.randn(TC, 9 * TC, generator=g) * 0.05)
    tab = torch.cat([w[0], w[1], w[0]], 1).contiguous().cuda()
    tail, ntab, tx = (_split(torch.randn(TN * TC, generator=g) * 0.05).cuda() for _ in range(3))
    b2, b3, bn = (torch.randn(c, generator=g).cuda() for c in (TC, TN, TC))
    mm, mo, mn = (torch.randint(0, 256, (TP * c // 8,), generator=g, dtype=torch.uint8).cuda() for c in (TC, TN, TC))
    return dict(src=src, x=x, res=res, tab=tab, tail=tail, ntab=ntab, tx=tx, b2=b2, b3=b3, bn=bn, mm=mm, mo=mo, mn=mn)


def _run_tail(form, direction):
    L, lib = _lib()
    o = _tail_operands()
    nxt, xs, backward = form.startswith('next'), form.endswith('xs'), direction == 'bwd'
    d = L.ConvTailDesc()
    d.a_hi, d.a_lo, d.w_hi, d.w_lo = o['src'][0].data_ptr(), o['src'][1].data_ptr(), o['tab'].data_ptr(), o['tab'].data_ptr() + 2 * 9 * TC
    d.t_hi, d.t_lo = o['tail'][0].data_ptr(), o['tail'][1].data_ptr()
    d.batch, d.h, d.w, d.c_mid, d.ldw = TB, TH, TH, TC, 3 * 9 * TC
    for i in range(9):
        d.tap_dy[i], d.tap_dx[i] = (1 - i // 3, 1 - i % 3) if backward else (i // 3 - 1, i % 3 - 1)
    ins, outs = [o['src'], o['tab'], o['tail']], {}
    outs['dst'], d.dst_hi, d.dst_lo = _pair_out(TP * TN)
    if xs:
        d.x_hi, d.x_lo, d.tx_hi, d.tx_lo = o['x'][0].data_ptr(), o['x'][1].data_ptr(), o['tx'][0].data_ptr(), o['tx'][1].data_ptr()
        ins += [o['x'], o['tx']]
    else:
        d.res_hi, d.res_lo = o['res'][0].data_ptr(), o['res'][1].data_ptr()
        ins.append(o['res'])
    if backward:
        d.mask_mid, d.mask_out = o['mm'].data_ptr(), o['mo'].data_ptr()
        ins += [o['mm'], o['mo']]
    else:
        outs['sign_mid'], outs['sign_out'] = _sentinel(TP * TC // 8, torch.uint8), _sentinel(TP * TN // 8, torch.uint8)
        d.bias_mid, d.bias_out, d.sign_mid, d.sign_out = o['b2'].data_ptr(), o['b3'].data_ptr(), outs['sign_mid'].data_ptr(), outs['sign_out'].data_ptr()
        d.relu_mid = d.relu_out = 1
        ins += [o['b2'], o['b3']]
    if nxt:
        outs['dstn'], d.dstn_hi, d.dstn_lo = _pair_out(TP * TC)
        d.n_hi, d.n_lo = o['ntab'][0].data_ptr(), o['ntab'][1].data_ptr()
        ins.append(o['ntab'])
        if backward:
            d.mask_next = o['mn'].data_ptr()
            ins.append(o['mn'])
        else:
            outs['sign_next'] = _sentinel(TP * TC // 8, torch.uint8)
            d.bias_next, d.sign_next, d.relu_next = o['bn'].data_ptr(), outs['sign_next'].data_ptr(), 1
            ins.append(o['bn'])
    L.check(lib.rart_conv3x3_tail_pair(ctypes.byref(d), L.stream_ptr()))
    torch.cuda.synchronize()
    return ins, outs


def run_case(case):
    """-> the recording's entry for the case: {'inputs': sha256, 'outputs': {buffer: sha256}}"""
    if case[0] == 'tail':
        inputs, outputs = _run_tail(*case[1:])
    elif case[0] == 'plain':
        inputs, outputs = _run_plain(*case[1:])
    else:
        inputs, outputs = _run_conv(*case)
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
