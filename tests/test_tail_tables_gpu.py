"""rart_conv3x3_tail_pair with the 1x1 expansion's fragment table staged in LDS once per workgroup (tables 1) against the same launch with
every wave loading it from L2 (tables 0): the same MFMAs in the same order, so every output is compared with torch.equal -- the pair
the kernel writes, the neighbour's reduction, and the sign tensors.  Staging stays at its default (the slab).

The cases and geometries are those of tests/test_tail_slab_gpu.py:
  2 x 9 x 11   a 128-position tile spans two images; M = 198 is no multiple of 128
  1 x 5 x 59   three tiles, the last one partial
  3 x 4 x 4    a single partial tile (waves 1 to 3 own few or no positions and still take every barrier of the chunk loop)
  1 x 3 x 60   one column too wide for the slab: the launch falls back to per-tap staging and direct tables under tables 1, and agrees
Every output buffer starts as NaN (sign tensors as 0xAA) and must come back finite."""
import ctypes

import pytest
import torch

from test_tail_slab_gpu import GEOMETRIES, MODES, _bits_of, _case

gpu = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


@gpu
@pytest.mark.parametrize('B,H,W', GEOMETRIES)
@pytest.mark.parametrize('mode', MODES)
def test_lds_tables_are_bit_identical_to_direct_tables(mode, B, H, W):
    from robustart_amd import _lib
    lib = _lib.load()
    d, out, keep = _case(_lib, mode, B, H, W)
    expect = {'dst'} | ({'dstn'} if mode.endswith('next') else set()) | (set() if mode.startswith('bwd') else {'sign_mid', 'sign_out'}) \
        | ({'sign_next'} if mode in ('fwd_next', 'xs_next') else set())
    assert set(out) == expect
    old = lib.rart_conv3x3_tail_pair_get_tables()
    got = {}
    try:
        for tables in (0, 1):
            _lib.check(lib.rart_conv3x3_tail_pair_set_tables(tables))
            for name, t in out.items():
                t.fill_(float('nan') if t.dtype == torch.bfloat16 else 0xAA)
            _lib.check(lib.rart_conv3x3_tail_pair(ctypes.byref(d), _lib.stream_ptr()))
            torch.cuda.synchronize()
            got[tables] = {name: t.clone() for name, t in out.items()}
    finally:
        lib.rart_conv3x3_tail_pair_set_tables(old)
    for name in sorted(out):
        for tables in (0, 1):
            if out[name].dtype == torch.bfloat16:
                assert torch.isfinite(got[tables][name].float()).all(), (name, tables)
        assert torch.equal(_bits_of(got[1][name]), _bits_of(got[0][name])), name
    assert not (got[1]['dst'].float() == 0).all()
    assert got[0]['dst'].float().abs().max().item() > 0.1          # a launch that wrote zeros everywhere would pass the lines above


@gpu
def test_engine_forward_backward_is_bit_identical_under_both_table_modes():
    """ResNet50Engine(precision='fp32x').forward_backward on 3 x 3 x 96 x 128 (layer1 at 24 x 32: six tail launches on the slab path, tiles
    that span images) with tables 0 and 1: torch.equal logits and input gradient."""
    from robustart_amd import _lib
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    lib = _lib.load()
    torch.manual_seed(0)
    m = randomize_bn_stats(get_model({'type': 'resnet50_official'}), 0).eval().cuda()
    for p in m.parameters():
        p.requires_grad_(False)
    eng = ResNet50Engine(m, 'cuda', precision='fp32x')
    assert eng.fused_tail_pair
    g = torch.Generator().manual_seed(43)
    x = torch.rand(3, 3, 96, 128, generator=g).cuda()
    y = torch.randint(0, 1000, (3,), generator=g).cuda()
    old = lib.rart_conv3x3_tail_pair_get_tables()
    res = {}
    try:
        for tables in (0, 1):
            _lib.check(lib.rart_conv3x3_tail_pair_set_tables(tables))
            logits, _, grad, _ = eng.forward_backward(x, MEAN, STD, y, 0)
            res[tables] = (logits.clone(), grad.clone())
    finally:
        lib.rart_conv3x3_tail_pair_set_tables(old)
    assert torch.isfinite(res[1][0]).all() and torch.isfinite(res[1][1]).all()
    assert torch.equal(res[1][0], res[0][0])
    assert torch.equal(res[1][1], res[0][1])
