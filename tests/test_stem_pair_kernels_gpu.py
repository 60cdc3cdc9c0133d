"""Kernel-level tests of the two fused reference-precision stem kernels (robustart_amd/csrc/stem_pair.hip) at sizes the engine's
`_forward` never reaches (it only takes multiples of 32, which always give whole tiles).

Forward, rart_engine_stem_fwd_fused_pair: the pooled pair, the argmax codes and the sign bits, bit for bit against the chain it replaces
(rart_engine_prep_input -> rart_gemm_pair_bf16 -> rart_engine_maxpool_pair, the engine's `fused_stem_fwd = False` path).  The chain takes
every multiple of 4, so all three sizes are checked that way; none needed the fp64 comparison.

Backward, rart_engine_stem_bwd_fused_pair, called through ctypes: at 256 x 256 against the chain rart_engine_maxpool_bwd_pair -> patches
GEMM -> rart_engine_stem_col2im_f32 at the bound of the engine test (relative L2 and maximum <= 2e-6 of scale).  The chain's col2im
takes only h % 16 == 0 and w % 32 == 0, so 4 x 4 and 36 x 44 (and 256 x 256 once more) are checked against an fp64 evaluation of the
same pair operands instead: the pool backward summed in fp32 and rounded to a hi + lo pair as the kernel rounds it, then the
kernel's three products (lo.hi + hi.lo + hi.hi) of that pair with the weight pair as a transposed convolution in fp64 -- what is left
is fp32 accumulation alone, inside the 2e-6 of scale that bounds the pair GEMM in tests/test_engine_x3_gpu.py.  (With the dropped lo.lo
products in the reference the distance is 2.4e-6 - 3.5e-6 relative L2: they are 2^-18 of a product and the sums are short.)  Because neither bound can see a
changed summation order, the SHA-256 of the gradient bytes is compared with tests/golden/stem_bwd_pair_digest.json, recorded from the
kernel as it stood before its pooled tile was re-laid-out, its stage loads were hoisted and its weights went through LDS
(tests/golden/make_stem_bwd_pair_digest.py).  The fp64 reference copies the kernel's choice of products, so at 4 x 4 and 36 x 44 it is
less independent than the chain: an error in WHICH products are formed would show only at 256 x 256 and in the digest.

Sizes (n, h, w):
  (1, 4, 4)      one tile, almost all of it outside the image
  (2, 36, 44)    pooled grid 9 x 11: one whole forward tile and partial tiles in both directions; 2 x 2 backward tiles, three of them partial
  (5, 256, 256)  320 forward tiles on the 256-workgroup grid: 64 workgroups take a second tile (the loop-carried source load), the others
                 do not
"""
import ctypes
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
SIZES = [(1, 4, 4), (2, 36, 44), (5, 256, 256)]
CODES = ['random', 'dead', 'centre']
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stem_bwd_pair_digest.json')


@pytest.fixture(scope='module')
def eng():
    from robustart_amd.model import get_model
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.model.resnet_torch import randomize_bn_stats
    torch.manual_seed(0)
    m = randomize_bn_stats(get_model({'type': 'resnet50_official'}), 0).eval()
    return ResNet50Engine(m, 'cuda', precision='fp32x')


def _stem_fwd(eng, x, u8, outs, fused):
    n, h, w = (x.shape[0], x.shape[1], x.shape[2]) if u8 else (x.shape[0], x.shape[2], x.shape[3])
    eng.fused_stem_fwd = fused
    try:
        acts = {}
        p1, _, sign = eng._stem_fwd(x, u8, MEAN, STD, n, h, w, outs, outs, acts)
        torch.cuda.synchronize()
        return [t.clone() for t in (p1, acts['p1_argmax'], sign) if t is not None]
    finally:
        eng.fused_stem_fwd = True


@pytest.mark.parametrize('outs', [True, False], ids=['codes+signs', 'pooled-only'])
@pytest.mark.parametrize('u8', [False, True], ids=['fp32', 'uint8'])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%dx%d' % s)
def test_stem_fwd_pair_is_bit_identical_to_the_chain(eng, size, u8, outs):
    n, h, w = size
    g = torch.Generator().manual_seed(100 + h)
    if u8:
        x = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).cuda()
    else:
        x = torch.rand(n, 3, h, w, generator=g).cuda()
    got = _stem_fwd(eng, x, u8, outs, True)
    want = _stem_fwd(eng, x, u8, outs, False)
    assert len(got) == len(want) == (3 if outs else 1)
    assert got[0].abs().max().item() > 0
    for name, a, b in zip(('pooled pair', 'argmax codes', 'sign bits'), got, want):
        assert a.shape == b.shape and torch.equal(a, b), name


def stem_bwd_case(size, codes):
    """-> (pooled gradient pair [2][n][h/4][w/4][64] bf16, argmax codes [n][h/4][w/4][64] uint8) on the CPU, fixed seeds"""
    from robustart_amd.model.engine_base import pair
    n, h, w = size
    g = torch.Generator().manual_seed(7 * h + w + CODES.index(codes))
    dz = pair(torch.randn(n, h // 4, w // 4, 64, generator=g))
    if codes == 'random':                          # 0..8 = a window element, 15 = window maximum <= 0
        cd = torch.randint(0, 10, (n, h // 4, w // 4, 64), generator=g, dtype=torch.uint8)
        cd[cd == 9] = 15
    else:
        cd = torch.full((n, h // 4, w // 4, 64), 15 if codes == 'dead' else 4, dtype=torch.uint8)
    return dz, cd


def stem_bwd_table():
    """the [2][16][1024] bf16 weight table pair of a fixed random 7 x 7 stem (no model behind it: the digest depends on nothing else)"""
    from robustart_amd.model.engine import ResNet50Engine
    from robustart_amd.model.engine_base import pair
    return pair(ResNet50Engine._stem_bwd_table(stem_bwd_weights(), dtype=torch.float32))


def stem_bwd_direct(size, codes, table):
    """rart_engine_stem_bwd_fused_pair through ctypes -> the fp32 gradient [n][3][h][w] on the CPU"""
    from robustart_amd import _lib
    lib = _lib.load()
    n, h, w = size
    dz, cd = stem_bwd_case(size, codes)
    dz, cd, table = dz.cuda(), cd.cuda(), table.cuda()
    grad = torch.full((n, 3, h, w), float('nan'), device='cuda')
    stdf = (ctypes.c_float * 3)(*STD)
    _lib.check(lib.rart_engine_stem_bwd_fused_pair(_lib.ptr(dz[0]), _lib.ptr(dz[1]), _lib.ptr(cd), _lib.ptr(table[0]), _lib.ptr(table[1]),
                                                   _lib.ptr(grad), n, h, w, stdf, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return grad.cpu()


def digest_key(size, codes):
    return '%dx%dx%d-%s' % (size + (codes,))


def digest(grad):
    return hashlib.sha256(grad.contiguous().numpy().tobytes()).hexdigest()


def stem_bwd_weights():
    g = torch.Generator().manual_seed(5)
    return torch.randn(64, 3, 7, 7, generator=g) * 0.1


def _pair64(t):
    """fp32 -> the (hi, lo) bf16 pair the engine stores, as two float64 tensors"""
    hi = t.to(torch.bfloat16)
    return hi.double(), (t - hi.float()).to(torch.bfloat16).double()


def stem_bwd_fp64(size, codes):
    """fp64 evaluation of the three products the kernel forms (x_lo.w_hi + x_hi.w_lo + x_hi.w_hi; lo.lo is dropped by design and, at
    2^-18 of a product, would alone be 2.7e-6 of scale here) on the pair operands it multiplies -> [n][3][h][w] float64 (CPU)"""
    n, h, w = size
    dz, cd = stem_bwd_case(size, codes)
    h2, w2 = h // 4, w // 4
    dv = dz[0].float() + dz[1].float()                              # hi + lo is exact in fp32
    z = torch.zeros(n, 2 * h2 + 2, 2 * w2 + 2, 64)                  # stem-output grid with one ring: element (ky, kx) of window q is 2q + k
    for k in range(9):
        ky, kx = divmod(k, 3)
        z[:, ky:ky + 2 * h2:2, kx:kx + 2 * w2:2] += torch.where(cd == k, dv, torch.zeros(()))
    xh, xl = _pair64(z[:, 1:1 + 2 * h2, 1:1 + 2 * w2])             # the ring lies outside the grid: no gradient goes there
    wh, wl = _pair64(stem_bwd_weights())
    ct = lambda x, wt: torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2), wt, stride=2, padding=3, output_padding=1)   # noqa: E731
    g = ct(xh + xl, wh) + ct(xh, wl)
    return g / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)


@pytest.mark.parametrize('codes', CODES)
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%dx%d' % s)
def test_stem_bwd_pair_vs_fp64_of_the_pair_operands(table, size, codes):
    got = stem_bwd_direct(size, codes, table).double()
    want = stem_bwd_fp64(size, codes)
    assert got.shape == want.shape and torch.isfinite(got).all()
    if codes == 'dead':                            # every window's maximum was <= 0: no gradient reaches the image
        assert not got.any() and not want.any()
        return
    rel = ((got - want).norm() / want.norm()).item()
    mx = ((got - want).abs().max() / want.abs().max()).item()
    print('stem backward pair vs fp64 %s %s: rel L2 %.2e, max %.2e of scale' % (size, codes, rel, mx))
    assert rel <= 2e-6 and mx <= 2e-6


@pytest.mark.parametrize('codes', CODES)
def test_stem_bwd_pair_matches_the_chain(eng, codes):
    size = n, h, w = SIZES[2]                      # the one size the chain's col2im accepts
    dz, cd = stem_bwd_case(size, codes)
    dz, cd = dz.cuda(), cd.cuda()
    out = []
    for fused in (True, False):
        eng.fused_stem_bwd = fused
        try:
            out.append(eng._stem_bwd({'in_shape': (n, h, w), 'p1_argmax': cd, 'y1': None}, dz, STD).clone())
        finally:
            eng.fused_stem_bwd = True
    torch.cuda.synchronize()
    a, b = out[0].double().flatten(), out[1].double().flatten()
    assert torch.isfinite(a).all()
    if codes == 'dead':
        assert not a.any() and not b.any()
        return
    rel = ((a - b).norm() / b.norm()).item()
    mx = ((a - b).abs().max() / b.abs().max()).item()
    print('stem backward pair vs chain %s %s: rel L2 %.2e, max %.2e of scale' % (size, codes, rel, mx))
    assert rel <= 2e-6 and mx <= 2e-6


@pytest.fixture(scope='module')
def table():
    return stem_bwd_table()


@pytest.mark.parametrize('codes', CODES)
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%dx%d' % s)
def test_stem_bwd_pair_gradient_bytes_match_the_recorded_digest(table, size, codes):
    want = json.load(open(DIGESTS))['sha256'][digest_key(size, codes)]
    grad = stem_bwd_direct(size, codes, table)
    assert torch.isfinite(grad).all()
    assert digest(grad) == want
