"""The row LayerNorm family and the ViT position add, bit for bit against a recording: rart_layernorm[_bwd]_{bf16,pair}
(csrc/row_norm.hip), rart_layernorm_bwd_full_bf16 (csrc/vit_bwd.hip) and rart_vit_add_pos_cls[_pair] (csrc/vit_aux.hip), all built
from csrc/rart_row_norm.h.  tests/golden/row_norm_bits.json was recorded by tests/golden/make_row_norm_bits.py from the commit BEFORE
the bf16 and the pair copies of these kernels were merged (the file names it); tests/test_row_kernels_gpu.py holds the same kernels
to fp64 bounds, this file holds them to "same operations, same order, same rounding points, same packer".

Per case the recording has a sha256 of the input bytes and one of every WHOLE output buffer: GUARD_ROWS rows behind what the call
names and the padding columns included, pre-filled with the bf16 NaN 0x7FA5 (fp32 buffers: 0x7FA57FA5), so a store outside the
contract changes the hash as well.  The inputs are rebuilt from the seeds of R.ln_case / R.rows_for; an input hash that differs
fails as "inputs drifted" before any kernel is blamed.  The recording is never remade after a kernel edit: a mismatch means the code
changed the arithmetic, and the fix goes into the code.

Cases:
  * LayerNorm forward and backward: every (rows, dim) of R.LN_SHAPES (dims on both sides of the slot-0 / slot-1 boundary, rows on
    both sides of the four-rows-per-workgroup boundary), both storages, dense strides and padded ones (inputs dim + 8, output
    dim + 16), the backward with and without the residual, and the ViT head's class-token strides of R.HEAD_SHAPE.
  * non-finite inputs, one forward and one backward case per storage at NONFINITE_SHAPE: +Inf in one row, a NaN in another (forward:
    both in x; backward: +Inf in res, whose element comes out +Inf, and the NaN in dy).  This pins what pack8's software rounding
    and split8's hardware convert make of non-finite results.  Every other row must equal the dense case's, bit for bit.
  * rart_layernorm_bwd_full_bf16: dims FULL_DIMS, rows 9 (a wave per row) and 1030 (the 512 walking waves take a second row, six of
    them a third), dx with a residual and dx null, accumulate 0 and 1 onto seeded dgamma / dbeta; dx, dgamma and dbeta are hashed.
  * rart_vit_add_pos_cls[_pair] at POS_SHAPES."""
import hashlib
import json
import os

import pytest
import torch

import _row_kernels_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'row_norm_bits.json')
PRECS = ('bf16', 'pair')
SENT = 0x7FA5                                       # a bf16 NaN
SENT32 = 0x7FA57FA5                                 # the same bytes as an fp32 NaN
GUARD_ROWS = 3
NONFINITE_SHAPE = (9, 768)
INF_AT, NAN_AT = (5, 3), (6, 700)                   # ordinary rows of R.rows_for: not planted, not the copy of row 0
INF_BITS, NAN_BITS = 0x7F80, 0x7FC0
FULL_DIMS = (8, 520, 768, 1024)
FULL_ROWS = (9, 1030)
POS_SHAPES = ((3, 5, 768), (2, 3, 8))


def _cases():
    out = []
    head = (R.HEAD_SHAPE[0], R.HEAD_SHAPE[2], 'head')
    for prec in PRECS:
        shapes = [(r, d, lay) for r, d in R.LN_SHAPES for lay in ('dense', 'padded')] + [head]
        out += [('ln_fwd', prec) + s for s in shapes] + [('ln_fwd', prec) + NONFINITE_SHAPE + ('nonfinite',)]
        out += [('ln_bwd', prec) + s + (res,) for s in shapes for res in (('res', 'nores') if s[2] != 'head' else ('nores',))]
        out += [('ln_bwd', prec) + NONFINITE_SHAPE + ('nonfinite', 'res')]
    out += [('ln_bwd_full', rows, dim, dx, 'acc%d' % acc) for dim in FULL_DIMS for rows in FULL_ROWS for dx in ('dx_res', 'nodx')
            for acc in (0, 1)]
    out += [('add_pos', prec) + s for prec in PRECS for s in POS_SHAPES]
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


def _sentinel(rows, ld):
    return torch.full((rows, ld), SENT, dtype=torch.int16, device='cuda').view(torch.bfloat16)


def _in_planes(v, prec, ld):
    """stored fp32 values [rows][cols] on the CPU -> the device planes [rows][ld], NaN from column cols on"""
    out = []
    for p in R.planes(v, prec):
        buf = torch.full((v.shape[0], ld), R.NAN, dtype=torch.bfloat16)
        buf[:, :v.shape[1]] = p
        out.append(buf.cuda())
    return out


def _plant(pl, at, bits):
    """one element of the stored operand becomes `bits` (hi plane; the lo plane of a pair holds +0 there)"""
    _bits(pl[0])[at] = bits
    for p in pl[1:]:
        _bits(p)[at] = 0


def _out_planes(rows, ld, prec):
    return [_sentinel(rows + GUARD_ROWS, ld) for _ in range(1 if prec == 'bf16' else 2)]


def _ptrs(L, pl):
    return [L.ptr(p) for p in pl]


def _named(prefix, pl):
    return dict(zip([prefix] if len(pl) == 1 else [prefix + '_hi', prefix + '_lo'], pl))


def _ln_operands(prec, rows, dim, layout):
    """-> the case, its stored x / dy / res [rows][dim], and the row strides of dy, x, res, dx and of the forward's output"""
    if layout == 'head':
        B, T, D = R.HEAD_SHAPE
        c = R.ln_case(6, D, prec)
        return c, {k: c[k][:B] for k in ('x', 'dy', 'res')}, dict(dy=D, x=T * D, res=0, dx=T * D, out=D)
    c = R.ln_case(rows, dim, prec)
    pad_in, pad_out = (8, 16) if layout == 'padded' else (0, 0)
    return c, c, dict(dy=dim + pad_in, x=dim + pad_in, res=dim + pad_in, dx=dim + pad_out, out=dim + pad_out)


def _run_ln_fwd(prec, rows, dim, layout):
    L, lib = _lib()
    c, v, s = _ln_operands(prec, rows, dim, layout)
    xd, g, b = _in_planes(v['x'], prec, s['x']), c['gamma'].cuda(), c['beta'].cuda()
    if layout == 'nonfinite':
        _plant(xd, INF_AT, INF_BITS)
        _plant(xd, NAN_AT, NAN_BITS)
    out = _out_planes(rows, s['out'], prec)
    fn = lib.rart_layernorm_bf16 if prec == 'bf16' else lib.rart_layernorm_pair
    L.check(fn(*_ptrs(L, xd), L.ptr(g), L.ptr(b), *_ptrs(L, out), rows, dim, s['x'], s['out'], R.EPS, L.stream_ptr()))
    return xd + [g, b], _named('out', out)


def _run_ln_bwd(prec, rows, dim, layout, res):
    L, lib = _lib()
    c, v, s = _ln_operands(prec, rows, dim, layout)
    dyd, xd, g = _in_planes(v['dy'], prec, s['dy']), _in_planes(v['x'], prec, s['x']), c['gamma'].cuda()
    rd = _in_planes(v['res'], prec, s['res']) if res == 'res' else [None] * len(xd)
    if layout == 'nonfinite':
        _plant(rd, INF_AT, INF_BITS)
        _plant(dyd, NAN_AT, NAN_BITS)
    out = _out_planes(rows, s['dx'], prec)
    fn = lib.rart_layernorm_bwd_bf16 if prec == 'bf16' else lib.rart_layernorm_bwd_pair
    L.check(fn(*_ptrs(L, dyd), *_ptrs(L, xd), L.ptr(g), *_ptrs(L, rd), *_ptrs(L, out), rows, dim, s['dy'], s['x'],
               s['res'] if res == 'res' else 0, s['dx'], R.EPS, L.stream_ptr()))
    return dyd + xd + [g] + rd, _named('dx', out)


def _run_ln_bwd_full(rows, dim, dx, acc):
    L, lib = _lib()
    c = R.ln_case(rows, dim, 'bf16')
    dyd, xd, rd = (_in_planes(c[k], 'bf16', dim)[0] for k in ('dy', 'x', 'res'))
    g = c['gamma'].cuda()
    pre = torch.randn(2, dim, generator=torch.Generator().manual_seed(400000 + 1000 * rows + dim))
    dgb = torch.full((2, dim + 8), SENT32, dtype=torch.int32).view(torch.float32)          # dgamma, dbeta and a guard of 8 behind each
    accumulate = int(acc[-1])
    if accumulate:
        dgb[:, :dim] = pre
    dgb = dgb.cuda()
    with_dx = dx == 'dx_res'
    out = _sentinel(rows + GUARD_ROWS, dim) if with_dx else None
    need = lib.rart_layernorm_bwd_workspace_bytes(dim)
    ws = torch.full((need,), 255, dtype=torch.uint8, device='cuda')                       # NaN as fp32
    inputs = [dyd, xd, g, rd if with_dx else None, dgb.clone()]
    L.check(lib.rart_layernorm_bwd_full_bf16(L.ptr(dyd), L.ptr(xd), L.ptr(g), L.ptr(rd if with_dx else None), L.ptr(out), rows, dim,
                                             dim, dim, dim if with_dx else 0, dim, R.EPS, L.ptr(dgb[0]), L.ptr(dgb[1]), accumulate,
                                             L.ptr(ws), need, L.stream_ptr()))
    outputs = dict(dgamma=dgb[0], dbeta=dgb[1])
    if with_dx:
        outputs['dx'] = out
    return inputs, outputs


def _run_add_pos(prec, B, T, D):
    L, lib = _lib()
    g = torch.Generator().manual_seed(300000 + 10000 * B + 1000 * T + D)
    x = R.store(torch.randn(B * T, D, generator=g), prec)
    cls, pos = torch.randn(D, generator=g).cuda(), torch.randn(T, D, generator=g).cuda()
    bufs = _out_planes(B * T, D, prec)
    for buf, p in zip(bufs, R.planes(x, prec)):
        buf[:B * T] = p.cuda()
    inputs = [b.clone() for b in bufs] + [cls, pos]
    fn = lib.rart_vit_add_pos_cls if prec == 'bf16' else lib.rart_vit_add_pos_cls_pair
    L.check(fn(*_ptrs(L, bufs), L.ptr(cls), L.ptr(pos), B, T, D, L.stream_ptr()))
    return inputs, _named('x', bufs)


RUNNERS = dict(ln_fwd=_run_ln_fwd, ln_bwd=_run_ln_bwd, ln_bwd_full=_run_ln_bwd_full, add_pos=_run_add_pos)


def run_case(case):
    """-> the recording's entry for the case: {'inputs': sha256, 'outputs': {buffer: sha256}}"""
    inputs, outputs = RUNNERS[case[0]](*case[1:])
    if 'nonfinite' in case:
        _, clean = RUNNERS[case[0]](*[f if f != 'nonfinite' else 'dense' for f in case[1:]])
        keep = [r for r in range(NONFINITE_SHAPE[0] + GUARD_ROWS) if r not in (INF_AT[0], NAN_AT[0])]
        for k in outputs:
            assert torch.equal(_bits(outputs[k])[keep], _bits(clean[k])[keep]), 'a planted row changed another row of %s' % k
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
