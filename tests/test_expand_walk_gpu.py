"""rart_expand_walk_pair (csrc/expand_walk_pair.hip): the short-K wide 1x1 pair launches of ResNet-50's identity blocks with the A rows
resident in registers, against rart_gemm_pair_bf16 on the same descriptor -- the same products in the same order and the same point-wise
tail, so the hi plane, the lo plane and the sign bytes are compared bit for bit.

Shapes: layer3's K = 256 -> N = 1024 at 2 x 14 x 14 = 392 rows (four / seven row tiles, the last one ragged) and 2 x 7 x 7 = 98 rows
(less than one 128-row tile), both row tiles of the entry, the columns of a row tile in one, two and four workgroups; the K = 128 -> 512
instance; the engine with the switch on and off."""
import ctypes
import functools

import pytest
import torch

gpu = pytest.mark.gpu
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
GP_RELU = 1


@functools.lru_cache(maxsize=None)
def _case(hw, K, N):
    """operands of one launch, made once: source pair, [hi | lo | hi] table, bias, skip / gradient pair, 1-bit mask"""
    from robustart_amd.model.engine_base import pair
    g = torch.Generator().manual_seed(100 * hw + K + N)
    M = 2 * hw * hw
    w = pair(torch.randn(N, K, generator=g) * 0.05)
    return dict(hw=hw, M=M, K=K, N=N, a=pair(torch.randn(M, K, generator=g)).cuda(), tab=torch.cat([w[0], w[1], w[0]], 1).contiguous().cuda(),
                bias=torch.randn(N, generator=g).cuda(), res=pair(torch.randn(M, N, generator=g)).cuda(),
                mask=torch.randint(0, 256, (M * N // 8,), generator=g, dtype=torch.uint8).cuda())


def _desc(c, form, dst, sign):
    """'fwd': bias + skip pair + ReLU + sign bytes; 'eval': the same without sign bytes; 'bwd': no bias, residual pair, 1-bit mask in"""
    from robustart_amd.model.engine_base import gemm_pair_desc
    fwd, hw = form != 'bwd', (c['hw'], c['hw'])
    return gemm_pair_desc(c['a'], c['tab'], dst, c['N'], c['K'], 3 * c['K'], c['N'], c['N'], bias=c['bias'] if fwd else None, res=c['res'],
                          mask_bits=None if fwd else c['mask'], sign_out=sign if form == 'fwd' else None, flags=GP_RELU if fwd else 0,
                          w_lo_off=c['K'], batch=2, grid=hw, src_hw=hw, k_per_tap=c['K'], taps=[(0, 0)], dst_hw=hw)


def _run(entry, c, form):
    from robustart_amd import _lib
    dst = torch.full((2, c['M'], c['N']), float('nan'), dtype=torch.bfloat16, device='cuda')
    sign = torch.full((c['M'] * c['N'] // 8,), 0xA5, dtype=torch.uint8, device='cuda')
    _lib.check(entry(ctypes.byref(_desc(c, form, dst, sign))))
    torch.cuda.synchronize()
    return dst, sign


@functools.lru_cache(maxsize=None)
def _want(hw, K, N, form):
    """rart_gemm_pair_bf16's output, computed once per case"""
    from robustart_amd import _lib
    lib = _lib.load()
    return _run(lambda d: lib.rart_gemm_pair_bf16(d, _lib.stream_ptr()), _case(hw, K, N), form)


@gpu
@pytest.mark.parametrize('tile_rows,col_parts', [(128, 1), (64, 1), (0, 0), (128, 2), (128, 4), (64, 4)])
@pytest.mark.parametrize('form', ['fwd', 'eval', 'bwd'])
@pytest.mark.parametrize('hw,K,N', [(14, 256, 1024), (7, 256, 1024), (14, 128, 512)])
def test_expand_walk_equals_gemm_pair(hw, K, N, form, tile_rows, col_parts):
    from robustart_amd import _lib
    lib = _lib.load()
    assert lib.rart_expand_walk_pair_max_k() >= K
    want, want_sign = _want(hw, K, N, form)
    got, got_sign = _run(lambda d: lib.rart_expand_walk_pair(d, tile_rows, col_parts, _lib.stream_ptr()), _case(hw, K, N), form)
    assert torch.isfinite(want.float()).all()                       # every element was written
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16))
    assert torch.equal(got[1].view(torch.int16), want[1].view(torch.int16))
    assert torch.equal(got_sign, want_sign)                         # 'eval' / 'bwd': untouched by both
    if form == 'fwd':
        assert not (want_sign == 0xA5).all()


@gpu
def test_column_count_must_be_a_multiple_of_64():
    """the entry walks whole 64-column chunks: N = 96 is refused before any launch, the destination stays untouched"""
    from robustart_amd import _lib
    lib = _lib.load()
    c = dict(_case(7, 256, 1024))
    c['N'] = 96
    dst = torch.full((2, c['M'], 96), float('nan'), dtype=torch.bfloat16, device='cuda')
    d = _desc(c, 'eval', dst, None)
    assert lib.rart_expand_walk_pair(ctypes.byref(d), 0, 0, _lib.stream_ptr()) != 0
    assert 'multiple of 64' in lib.rart_last_error_string().decode()
    torch.cuda.synchronize()
    assert torch.isnan(dst.float()).all()


@gpu
def test_engine_switch_is_bit_identical():
    """B = 2 ResNet-50 gradient evaluation in reference precision with `expand_walk_pair` on and off: the same logits and input gradient,
    and the switch does move the identity-block launches of layer2 and layer3 to the new entry"""
    from robustart_amd.model import get_model
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    from robustart_amd.model.engine import ResNet50Engine
    torch.manual_seed(0)
    m = randomize_bn_stats(get_model({'type': 'resnet50_official'})).eval()
    eng = ResNet50Engine(m, 'cuda', precision='fp32x')
    assert eng.expand_walk_max_k >= 256
    eng.expand_walk_pair = True
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(2, 3, 64, 64, generator=g).cuda(), torch.tensor([1, 2]).cuda()
    walked = []
    entry = eng.lib.rart_expand_walk_pair

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name == 'rart_expand_walk_pair':
                return lambda *a: (walked.append(1), entry(*a))[1]
            return getattr(self._lib, name)
    lib = eng.lib
    eng.lib = Spy(lib)
    on = eng.forward_backward(x, MEAN, STD, y, 0)
    on = (on[0].clone(), on[2].clone())
    assert len(walked) == 16             # layer2's three and layer3's five identity blocks: the expansion and conv1^T each
    eng.lib = lib
    eng.expand_walk_pair = False
    off = eng.forward_backward(x, MEAN, STD, y, 0)
    assert len(walked) == 16
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[2])
    assert torch.isfinite(on[0]).all() and on[1].abs().max() > 0
