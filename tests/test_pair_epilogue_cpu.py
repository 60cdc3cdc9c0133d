"""The conv instances of the pair GEMM are compiled without the GELU forms (gp_finish_segment<true, false>, csrc/rart_gemm_pair_dev.h): a
conv-mode descriptor that sets one is refused with RART_ERR_INVALID by every entry, launching or planning, before any HIP call; plain
products keep all three.  Runs without a GPU (the refusal precedes the launch; the plan entry launches nothing)."""
import ctypes

import pytest

from robustart_amd import _lib

GELU, GELU_BWD, GELU_KEEP = 4, 8, 64


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _desc(conv, flags):
    d = _lib.GemmPairClsDesc()
    o = d.two.one
    for name in ('a_hi', 'a_lo', 'w_hi', 'w_lo', 'dst_hi', 'dst_lo', 'aux_hi', 'aux_lo'):
        setattr(o, name, 4096)                  # (never dereferenced: nothing is launched)
    o.M, o.N, o.K, o.lda, o.ldw, o.ldc, o.w_rows, o.flags = 392, 128, 64, 64, 64, 128, 128, flags
    if conv:
        o.conv, o.batch, o.grid_h, o.grid_w, o.src_h, o.src_w, o.sy, o.sx, o.k_per_tap, o.n_taps = 1, 2, 14, 14, 14, 14, 1, 1, 64, 1
        o.dst_h, o.dst_w, o.dst_sy, o.dst_sx = 14, 14, 1, 1
    return d


@pytest.mark.parametrize('flag', [GELU, GELU_BWD, GELU_KEEP])
def test_conv_mode_refuses_the_gelu_forms(lib, flag):
    d = _desc(True, flag)
    plan = _lib.GemmPairPlan()
    for st in (lib.rart_gemm_pair_plan_bf16(ctypes.byref(d), 256, ctypes.byref(plan)), lib.rart_gemm_pair_bf16(ctypes.byref(d.two.one), None)):
        assert st == 1 and b'GELU forms are served by plain products only' in lib.rart_last_error_string()


@pytest.mark.parametrize('flag', [0, GELU, GELU_BWD, GELU_KEEP])
def test_plain_products_keep_them_and_conv_mode_its_other_flags(lib, flag):
    plan = _lib.GemmPairPlan()
    assert lib.rart_gemm_pair_plan_bf16(ctypes.byref(_desc(False, flag)), 256, ctypes.byref(plan)) == 0 and plan.n_launches >= 1
    if flag == 0:
        assert lib.rart_gemm_pair_plan_bf16(ctypes.byref(_desc(True, 1)), 256, ctypes.byref(plan)) == 0 and plan.n_launches == 1
