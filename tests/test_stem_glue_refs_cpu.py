"""CPU checks of tests/_stem_glue_ref.py, the references tests/test_stem_glue_kernels_gpu.py holds csrc/engine_aux.hip (both
storages) to.  The pool references (torch's max_pool2d and its autograd on the CPU) agree with a triple-loop model
written from the header's words -- first maximum in scan order, code 15 where the window maximum is not > 0 --, col2im_ref with a loop
over (r, s, p, q), prep_ref with (x - mean) / std in fp64.  The generated inputs have the properties the GPU tests rely on, so that
no test can pass on a degenerate draw: enough tied windows, every code in every class of window, a wrong tie rule or a comparison of
the hi planes alone visible in the reference itself, lattice sums exact in fp32, pairs stable under re-splitting."""
import numpy as np
import pytest
import torch

import _stem_glue_ref as R

U32 = 2.0 ** -24


def test_split_is_the_suites_split():
    from test_mixer_gpu import _split
    v = torch.randn(4, 33, generator=torch.Generator().manual_seed(0))
    assert torch.equal(R.split(v).view(torch.int16), _split(v).view(torch.int16))
    assert float(np.float32(1) / np.float32(255)) == float(np.float32(1 / 255))           # the u8 scale: either way of writing it


# ------------------------------------------------------------------ max pool
def _pool_model(x):
    """the header's words, one window at a time -> pooled, codes"""
    n, c, h, w = x.shape
    pooled = torch.empty(n, c, h // 2, w // 2, dtype=x.dtype)
    codes = torch.empty(n, c, h // 2, w // 2, dtype=torch.uint8)
    xl = x.tolist()
    for i in range(n):
        for ch in range(c):
            for oy in range(h // 2):
                for ox in range(w // 2):
                    best, code = float('-inf'), 0
                    for ky in range(3):
                        for kx in range(3):
                            y, xx = 2 * oy - 1 + ky, 2 * ox - 1 + kx
                            if 0 <= y < h and 0 <= xx < w and xl[i][ch][y][xx] > best:
                                best, code = xl[i][ch][y][xx], ky * 3 + kx
                    pooled[i, ch, oy, ox] = best
                    codes[i, ch, oy, ox] = code if best > 0 else 15
    return pooled, codes


def _pool_bwd_model(x, codes, dpool):
    """dz = (x > 0) * sum of dpool over the windows whose code names this pixel"""
    n, c, h, w = x.shape
    dz = torch.zeros_like(x)
    for i in range(n):
        for ch in range(c):
            for oy in range(h // 2):
                for ox in range(w // 2):
                    code = int(codes[i, ch, oy, ox])
                    if code != 15:
                        dz[i, ch, 2 * oy - 1 + code // 3, 2 * ox - 1 + code % 3] += dpool[i, ch, oy, ox]
    return torch.where(x > 0, dz, torch.zeros_like(dz))


@pytest.mark.parametrize('h,w', [(2, 2), (2, 8), (6, 8)])
@pytest.mark.parametrize('pair', [False, True])
def test_pool_refs_match_the_loop_model(h, w, pair):
    x = (R.lattice_pool_input_pair if pair else R.lattice_pool_input)(2, h, w, 8, 17 + h + w).double()
    pooled, codes, sign = R.maxpool_ref(x)
    want_pooled, want_codes = _pool_model(x)
    assert torch.equal(pooled.view(torch.int64), want_pooled.view(torch.int64))            # bits: the sign of a zero maximum too
    assert torch.equal(codes, want_codes)
    assert torch.equal(codes, R.window_codes(x, 'first'))
    bits = R.nhwc(want_pooled > 0)
    for j in range(8):
        assert torch.equal((sign[..., 0] >> j) & 1, bits[..., j].to(torch.uint8))
    dpool = R.lattice_grad_bf16(pooled.shape, 5)
    got = R.maxpool_bwd_ref(x, dpool)
    assert torch.equal(got, _pool_bwd_model(x, want_codes, dpool))
    assert got[x <= 0].abs().sum() == 0 and (got != 0).any()


def _classes(oh, ow):
    oy, ox = torch.meshgrid(torch.arange(oh), torch.arange(ow), indexing='ij')
    return {'corner': (oy == 0) & (ox == 0), 'top': (oy == 0) & (ox > 0), 'left': (oy > 0) & (ox == 0), 'interior': (oy > 0) & (ox > 0)}


@pytest.mark.parametrize('shape', R.POOL_SHAPES, ids=str)
@pytest.mark.parametrize('kind', R.POOL_KINDS)
def test_pool_inputs_are_not_degenerate(kind, shape):
    n, h, w, c = shape
    x = R.pool_case(kind, shape)
    pair = kind.endswith('pair')
    if pair:
        assert x.dtype == torch.float32
        p = R.split(x)
        assert torch.equal(p[0].float() + p[1].float(), x)                                 # hi + lo is the value, exactly
        assert torch.equal(R.split(p[0].float() + p[1].float()).view(torch.int16), p.view(torch.int16))      # canonical
    else:
        assert x.dtype == torch.float64 and torch.equal(x.to(torch.bfloat16).double(), x)                   # exact in bf16
    xd = x.double()
    pooled, codes, _ = R.maxpool_ref(xd)
    assert torch.equal(codes, R.window_codes(xd, 'first'))
    # every class of window that the size has shows every code its geometry allows, and code 15
    for cls, mask in _classes(h // 2, w // 2).items():
        if mask.any():
            seen = set(codes[:, :, mask].flatten().tolist())
            assert seen >= set(R.class_codes(cls) + [15]), (cls, sorted(seen))
    # zeros of both signs, a window of nonpositive values whose maximum is a zero, and one whose maximum is a negative number
    sign_bit = xd.view(torch.int64) < 0
    assert ((xd == 0) & ~sign_bit).any() and ((xd == 0) & sign_bit).any() == (not pair)      # a pair has no canonical -0
    assert (pooled == 0).any() and (pooled < 0).any() and (codes[pooled <= 0] == 15).all()
    if kind.startswith('lattice'):
        tied = R.tied_share(xd)
        last = (R.window_codes(xd, 'last') != codes).double().mean().item()
        assert tied >= 0.2 and last >= 0.1, (tied, last)
        if pair:
            hi_only = (R.maxpool_ref(R.split(x)[0].double())[1] != codes).double().mean().item()
            assert hi_only >= 0.1, hi_only


def test_large_lattices_tie_too():
    """the unplanted lattice of the grid-stride cases, at a small size: the same shares"""
    for pair in (False, True):
        x = R.lattice_pool_input_large(2, 16, 16, 16, 3, pair=pair)
        assert x.dtype == torch.float32 and R.tied_share(x.double()) >= 0.2
        if pair:
            p = R.split(x)
            assert torch.equal(R.split(p[0].float() + p[1].float()).view(torch.int16), p.view(torch.int16))
            assert (R.maxpool_ref(p[0].double())[1] != R.maxpool_ref(x.double())[1]).double().mean().item() >= 0.1
        else:
            assert torch.equal(x.to(torch.bfloat16).float(), x)


# ------------------------------------------------------------------ lattice gradients and patches
def test_lattice_gradients_sum_exactly():
    g = R.lattice_grad_bf16((4096, 16), 1)
    k = g * 8
    assert torch.equal(k, k.round()) and k.abs().max() == 64 and torch.equal(g.to(torch.bfloat16).double(), g)
    for terms in (4, 16):
        s = g[:, :terms].sum(1)
        assert torch.equal(s.float().double(), s)
    s4 = g[:, :4].sum(1)
    assert torch.equal(s4.to(torch.bfloat16).double(), s4)                                 # |k| <= 256: the pool backward rounds nothing
    p = R.lattice_grad_pair((4096, 16), 2)
    k = p * 2.0 ** 12
    assert torch.equal(k, k.round()) and k.abs().max() < 2 ** 15 and k.abs().max() > 2 ** 14
    sp = R.split(p.float())
    assert torch.equal(sp[0].double() + sp[1].double(), p)                                 # exact as a pair
    for terms in (4, 16):
        s = p[:, :terms].sum(1)
        assert torch.equal(s.float().double(), s)
    s4 = R.split(p[:, :4].sum(1).float())
    assert torch.equal(s4[0].double() + s4[1].double(), p[:, :4].sum(1))                   # 17 bits: hi's 8, lo's 8 and lo's sign


def test_canonical_pairs_are_stable():
    v = R.canonical(torch.randn(1 << 16, generator=torch.Generator().manual_seed(4)))
    p = R.split(v)
    assert torch.equal(p[0].float() + p[1].float(), v)
    assert torch.equal(R.split(v).view(torch.int16), p.view(torch.int16))


# ------------------------------------------------------------------ col2im
@pytest.mark.parametrize('std', [None, R.IMAGENET_STD], ids=['nostd', 'imagenet'])
def test_col2im_ref_matches_the_loop(std):
    n, h, w = 2, 16, 32
    patches = R.lattice_grad_pair((n, h // 2, w // 2, R.PATCH_COLS), 9)
    patches[..., 147:] = float('nan')
    want = torch.zeros(n, 3, h, w, dtype=torch.float64)
    taps = torch.zeros(h, w, dtype=torch.int64)
    for r in range(7):
        for s in range(7):
            for p in range(h // 2):
                for q in range(w // 2):
                    y, x = 2 * p - 3 + r, 2 * q - 3 + s
                    if 0 <= y < h and 0 <= x < w:
                        want[:, :, y, x] += patches[:, p, q, (r * 7 + s) * 3:(r * 7 + s) * 3 + 3]
                        taps[y, x] += 1
    assert int(taps.max()) == 16 and int(taps.min()) == 4                                  # interior pixels, and the corner ones
    s64 = R.col2im_sum64(patches)
    assert torch.equal(s64, want) and torch.equal(s64.float().double(), s64)
    istd = (np.float32(1) / np.asarray(std, np.float32)) if std is not None else np.ones(3, np.float32)
    assert torch.equal(R.col2im_ref(patches, std), want.float() * torch.from_numpy(istd).view(1, 3, 1, 1))
    for (p, q, col) in ((0, 0, 0), (0, 0, 30), (7, 15, 146), (3, 4, 77)):
        t = R.one_hot_target(p, q, col, h, w)
        one = torch.zeros(1, h // 2, w // 2, R.PATCH_COLS, dtype=torch.float64)
        one[0, p, q, col] = 3.0
        hit = R.col2im_sum64(one).nonzero().tolist()
        assert hit == ([] if t is None else [[0, t[0], t[1], t[2]]])


# ------------------------------------------------------------------ input preparation
@pytest.mark.parametrize('norm', [(None, None), (R.IMAGENET_MEAN, R.IMAGENET_STD)], ids=['nonorm', 'imagenet'])
@pytest.mark.parametrize('is_u8', [False, True])
def test_prep_ref_against_fp64(is_u8, norm):
    mean, std = norm
    n, h, w = 3, 32, 48
    if is_u8:
        src = R.prep_src_u8(n, h, w)
        for c in range(3):
            assert len(set(src[..., c].flatten().tolist())) == 256
    else:
        src, planted = R.prep_src_f32(n, h, w, mean, std, 11)
        assert min(planted) >= 40 and src.min() >= 0 and src.max() <= 1
    hi, lo = R.prep_ref(src, is_u8, mean, std)
    assert hi.shape == (n, h + 8, w + 8, 4) and hi.dtype == torch.bfloat16
    v64 = R.prep_v64(src, is_u8, mean, std)
    got = hi[:, 3:3 + h, 3:3 + w, :3].double() + lo[:, 3:3 + h, 3:3 + w, :3].double()
    ratio = ((got - v64).abs() / (2.0 ** -16 * v64.abs() + U32)).max().item()
    assert ratio <= 1.0, ratio
    for plane in (hi, lo):                                                                  # the border and channel 3: +0 bits
        border = plane.clone()
        border[:, 3:3 + h, 3:3 + w, :3] = 0
        assert (border.view(torch.int16) == 0).all()
    if not is_u8:
        # the planted values reach a rounding boundary from both sides: hi takes both neighbours, lo both signs near half an ulp
        hi_v, lo_v = hi[0, 3, 6:48, 0].double(), lo[0, 3, 6:48, 0].double()              # pixels 3 .. 44 of image 0, channel 0
        ulp = torch.pow(2.0, torch.floor(torch.log2(hi_v.abs())) - 7)
        near = lo_v.abs() >= 0.49 * ulp
        assert near.double().mean() >= 0.8 and (lo_v[near] > 0).any() and (lo_v[near] < 0).any(), (hi_v, lo_v)
