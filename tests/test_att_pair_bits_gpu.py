"""The fused pair attention, bit for bit against a recording: rart_vit_attention_pair and rart_vit_attention_bwd_pair
(csrc/vit_pair.hip), the one-item kernels (one workgroup per (image, head)) and the walking ones (one workgroup per CU, wave 7 a
loader).  tests/golden/att_pair_bits.json was recorded by tests/golden/make_att_pair_bits.py from the commit BEFORE the per-tile
arithmetic of the two forms was moved into shared helpers (the file names it).  tests/test_vit_x3_gpu.py holds these kernels to fp64
bounds and the walking form to the one-item form; both of those pass when the two forms change together, this file does not.

Per case the recording has a sha256 of the input bytes and one of every WHOLE output buffer, pre-filled with the bf16 NaN 0x7FA5 (the
fp32 statistics: 0x7FA57FA5), so an element the kernels leave out or a changed padding row of the statistics shows as well.  The
inputs come from seeded CPU generators and are split into hi + lo planes on the CPU; an input hash that differs fails as "inputs
drifted" before any kernel is blamed.  The backward's `out` operand is a seeded random pair, not the forward's result: the kernel
uses it in delta = rowsum(dO * O) alone, so the backward cases do not depend on the forward.  The recording is never remade after a
kernel edit: a mismatch means the code changed the arithmetic, and the fix goes into the code.

Cases (head_dim 64), forward and backward each:
  * the one-item kernels (RART_ATT_WALK=0), B = 2, H = 3 (not a power of two: the item arithmetic), at SMALL_T: every key-tile count
    1 .. 7 with a last tile of ONE key, and the counts 1, 2, 3, 5, 7 with a full last tile as well; 197 is ViT-B/16's own;
  * the walking kernels (variable unset) and the same shapes under RART_ATT_WALK=0, H = 12, at WALK_SHAPES: 86 x 12 = 1032 items is
    just above the 1024 that 256 CUs need (eight workgroups take a fifth item), 1200 and 1080 items give other uneven runs; 193 tokens
    is the smallest seventh tile, 224 a full one.  The walking cases assert B * H >= 4 * CUs, so a device on which these shapes would
    not walk fails loudly; both modes are held to the recording, in which they are equal (make_att_pair_bits.py checks that)."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'att_pair_bits.json')
SENT = 0x7FA5                                       # a bf16 NaN
SENT32 = 0x7FA57FA5                                 # the same bytes as an fp32 NaN
HD = 64
SMALL_B, SMALL_H = 2, 3
SMALL_T = (1, 31, 32, 33, 64, 65, 96, 97, 129, 160, 161, 193, 197, 224)
WALK_H = 12
WALK_SHAPES = ((86, 193), (100, 197), (90, 224))
ENV = 'RART_ATT_WALK'


def _cases():
    out = [(d, 'one', SMALL_B, SMALL_H, T) for T in SMALL_T for d in ('fwd', 'bwd')]
    out += [(d, mode, B, WALK_H, T) for B, T in WALK_SHAPES for d in ('fwd', 'bwd') for mode in ('walk', 'one')]
    return out


def case_id(case):
    return '-'.join(str(f) for f in case)


CASES = _cases()


def sha(tensors):
    """sha256 over the bytes of the tensors, in order"""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _split(t):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


_operands = {}


def operands(B, H, T):
    """-> the qkv, out and dout pairs of a shape on the device and the sha256 of the forward's and of the backward's inputs; built once
    per shape (the cases of one shape are neighbours in CASES) and never written"""
    key = (B, H, T)
    if key not in _operands:
        _operands.clear()
        D = H * HD
        g = torch.Generator().manual_seed(500000 + 1000 * B + 17 * H + T)
        qkv = _split(torch.randn(B * T, 3 * D, generator=g) * 1.5)
        dout = _split(torch.randn(B * T, D, generator=g) * 0.1)
        out = _split(torch.randn(B * T, D, generator=g))
        _operands[key] = dict(qkv=qkv.cuda(), out=out.cuda(), dout=dout.cuda(), fwd=sha([qkv]), bwd=sha([qkv, out, dout]))
    return _operands[key]


def _pair_of_sentinels(rows, cols):
    return torch.full((2, rows, cols), SENT, dtype=torch.int16, device='cuda').view(torch.bfloat16)


def _run(direction, B, H, T):
    from robustart_amd import _lib as L
    lib = L.load()
    D = H * HD
    ops = operands(B, H, T)
    qkv, sp = ops['qkv'], L.stream_ptr()
    if direction == 'fwd':
        out = _pair_of_sentinels(B * T, D)
        L.check(lib.rart_vit_attention_pair(L.ptr(qkv[0]), L.ptr(qkv[1]), L.ptr(out[0]), L.ptr(out[1]), B, T, H, HD, sp))
        outputs = dict(out=out)
    else:
        o, do = ops['out'], ops['dout']
        dqkv = _pair_of_sentinels(B * T, 3 * D)
        stats = torch.full((B * H * ((T + 31) // 32 * 32), 4), SENT32, dtype=torch.int32, device='cuda').view(torch.float32)
        L.check(lib.rart_vit_attention_bwd_pair(L.ptr(qkv[0]), L.ptr(qkv[1]), L.ptr(o[0]), L.ptr(o[1]), L.ptr(do[0]), L.ptr(do[1]),
                                                L.ptr(dqkv[0]), L.ptr(dqkv[1]), L.ptr(stats), B, T, H, HD, sp))
        outputs = dict(dqkv=dqkv, stats=stats)
    torch.cuda.synchronize()
    return ops[direction], outputs


def run_case(case):
    """-> the recording's entry for the case: {'inputs': sha256, 'outputs': {buffer: sha256}}"""
    direction, mode, B, H, T = case
    if mode == 'walk':
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        assert B * H >= 4 * cus, 'these shapes do not walk on a device of %d CUs: the walking kernels would go untested' % cus
    before = os.environ.get(ENV)                    # the library reads the variable at every call
    try:
        if mode == 'one':
            os.environ[ENV] = '0'
        else:
            os.environ.pop(ENV, None)
        inputs, outputs = _run(direction, B, H, T)
    finally:
        if before is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = before
    return {'inputs': inputs, 'outputs': {k: sha([v]) for k, v in outputs.items()}}


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
