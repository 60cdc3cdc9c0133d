"""The chain kernels of the ResNet-50 stem (csrc/engine_aux.hip: one kernel text per operation, instantiated for bf16 and for pair
storage), each against a plain reference of its own on the MI355X: rart_engine_prep_input, rart_engine_maxpool[_keep], rart_engine_maxpool_bwd, rart_engine_maxpool[_bwd]_pair,
rart_engine_stem_col2im[_f32].  The fused stem kernels are tested as bit-identical to these chains; this module is what the chains
themselves are held to.  The references and the inputs are in tests/_stem_glue_ref.py, pinned on the CPU by
tests/test_stem_glue_refs_cpu.py (the tie rule, the code 15, the shares of tied windows, the exactness of the lattice sums).

Conventions (those of tests/test_shared_train_kernels_gpu.py): calls go through robustart_amd._lib and the status is checked; every
launch is run twice and must be bit-identical; output buffers are pre-filled with NaN (byte outputs with 0xEE, which is no code), and
64 elements behind every output, and the gap between the planes of an output pair, hold the sentinel 777 (bytes: 0x77), which must
survive; what a kernel must not interpret is NaN: the gap between an input's hi and lo plane, patch columns 147..151.

Bit-exact checks (no tolerance): both planes of prep_input for fp32 and uint8 sources; the pooled bits (the sign of a zero maximum
included), the argmax codes and the sign bytes of the four pool forwards; the pair pool's output planes = the input planes at the
reference argmax; the pool backwards on lattice gradients (the fp64 sum cast to bf16, or split as a pair), their +0 wherever y <= 0
or the code is 15, and sum dz = sum of dpool over the windows whose code is not 15; col2im on lattice patches and on one-hot patches;
every case with more items than one launch holds (256 * 16 workgroups of 256 threads), where the references are fp32, which is exact
for these values.

Bounds of the randn cases (U = 2^-24, right-hand sides in fp64; terms = the <= 4 pooled gradients or <= 16 patch entries of a pixel):
  * rart_engine_maxpool_bwd: |dz - ref| <= ulp_bf16(ref) + 3 U sum|terms|       (three fp32 additions, one bf16 rounding)
  * rart_engine_maxpool_bwd_pair: |dz_hi + dz_lo - ref| <= 2^-16 |ref| + 3 U sum|terms|        (a re-split pair)
  * col2im: |got - istd ref| <= istd (16 U sum|terms| + U |ref|)                (fifteen fp32 additions, one multiplication)

Measured on the MI355X, worst |err| / bound of the randn cases (the same for the lattice and the relu(randn) pool input of a size):
  rart_engine_maxpool_bwd       (1, 2, 2, 8) 0.0000   (2, 2, 8, 8) 0.5000   (3, 6, 10, 64) 0.5000   (1, 16, 16, 24) 0.5000
  rart_engine_maxpool_bwd_pair  (1, 2, 2, 8) 0.0000   (2, 2, 8, 8) 0.3287   (3, 6, 10, 64) 0.4786   (1, 16, 16, 24) 0.4929
    (0 at 2 x 2: one window per channel, so a gradient is copied and nothing is added or rounded)
  rart_engine_stem_col2im       std null / ImageNet: (1, 16, 32) 0.0000 / 0.0535   (2, 32, 64) 0.0262 / 0.0484   (1, 48, 32) 0.0000 / 0.0535
  rart_engine_stem_col2im_f32   std null / ImageNet: (1, 16, 32) 0.1104 / 0.1374   (2, 32, 64) 0.1516 / 0.1573   (1, 48, 32) 0.1543 / 0.1558
Every bit-exact check holds.  Against a build of the two sources these kernels then had (one per storage) with seven deliberate,
memory-safe mistakes (>= in the bf16 pool's
comparison, code 15 only below zero in the pair pool, y < 0 as the backward's mask, the last window column skipped in the pair
backward, the tap at patch column 0 / the last patch row dropped in the two col2im kernels, a stride one too long in prep_input's loop)
53 of the 63 cases fail: every case but the small prep_input ones, the refusals and the pair forward's large case, which those
mistakes do not touch."""
import ctypes

import pytest
import torch

import _stem_glue_ref as R
from test_mixer_gpu import _ulp_bf16

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
NAN = float('nan')
SENT = 777.0                                        # exact in bf16 and fp32
TAIL = 64
BYTE_FILL, BYTE_SENT = 0xEE, 0x77
NORMS = [(None, None), (R.IMAGENET_MEAN, R.IMAGENET_STD)]
NORM_IDS = ['nonorm', 'imagenet']


def _lib():
    from robustart_amd import _lib as L
    return L, L.load()


def _c3(v):
    return None if v is None else (ctypes.c_float * 3)(*v)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _out(numel, dtype=torch.bfloat16):
    """NaN (bytes: 0xEE) in the leading numel elements, the sentinel in the TAIL behind them"""
    byte = dtype == torch.uint8
    buf = torch.full((numel + TAIL,), BYTE_SENT if byte else SENT, dtype=dtype, device='cuda')
    buf[:numel] = BYTE_FILL if byte else NAN
    return buf


def _tail_ok(buf, numel):
    return bool((buf[numel:] == (BYTE_SENT if buf.dtype == torch.uint8 else SENT)).all())


def _untouched(buf, numel):
    body = buf[:numel]
    return _tail_ok(buf, numel) and bool((body == BYTE_FILL).all() if buf.dtype == torch.uint8 else torch.isnan(body).all())


def _pair_in(planes, gap):
    """[hi | gap of NaN | lo] on the device -> the buffer and lo_off"""
    numel = planes[0].numel()
    buf = torch.full((2 * numel + gap,), NAN, dtype=torch.bfloat16)
    buf[:numel] = planes[0].reshape(-1)
    buf[numel + gap:] = planes[1].reshape(-1)
    return buf.cuda(), numel + gap


def _pair_out(numel, gap):
    """[hi NaN | gap of 777 | lo NaN | 777] -> the buffer and lo_off"""
    buf = torch.full((2 * numel + gap + TAIL,), SENT, dtype=torch.bfloat16, device='cuda')
    buf[:numel] = NAN
    buf[numel + gap:2 * numel + gap] = NAN
    return buf, numel + gap


def _pair_planes(buf, numel, gap):
    assert bool((buf[numel:numel + gap] == SENT).all()) and bool((buf[2 * numel + gap:] == SENT).all()), 'written outside the planes'
    return buf[:numel], buf[numel + gap:2 * numel + gap]


def _pair_untouched(buf, numel, gap):
    hi, lo = _pair_planes(buf, numel, gap)
    return bool(torch.isnan(hi).all() and torch.isnan(lo).all())


def _twice(run):
    """run() -> a tuple of device tensors; two runs, bit-identical"""
    a, b = run(), run()
    torch.cuda.synchronize()
    for s, t in zip(a, b):
        assert torch.equal(s.view(torch.uint8), t.view(torch.uint8)), 'second run differs'
    return a


# ------------------------------------------------------------------ rart_engine_prep_input
def _prep_run(src, is_u8, n, h, w, mean, std):
    L, lib = _lib()
    numel = n * (h + 8) * (w + 8) * 4
    hi, lo = _out(numel), _out(numel)
    L.check(lib.rart_engine_prep_input(L.ptr(src), 1 if is_u8 else 0, L.ptr(hi), L.ptr(lo), n, h, w, _c3(mean), _c3(std), L.stream_ptr()))
    assert _tail_ok(hi, numel) and _tail_ok(lo, numel)
    return hi[:numel], lo[:numel]


def _prep_check(src, is_u8, n, h, w, mean, std):
    want_hi, want_lo = R.prep_ref(src, is_u8, mean, std)
    dev = src.cuda()
    hi, lo = _twice(lambda: _prep_run(dev, is_u8, n, h, w, mean, std))
    assert torch.equal(_bits(hi).cpu(), _bits(want_hi).view(-1)), 'hi plane'
    assert torch.equal(_bits(lo).cpu(), _bits(want_lo).view(-1)), 'lo plane'


@pytest.mark.parametrize('norm', NORMS, ids=NORM_IDS)
@pytest.mark.parametrize('n,h,w', [(1, 1, 1), (2, 5, 7), (3, 32, 48)])
def test_prep_input_bit_exact(n, h, w, norm):
    """fp32 source: random in [0, 1] with 0, 1, mean[c] and values on either side of a bf16 rounding boundary of v planted; uint8
    source: every byte in every channel once the size holds 256 pixels (smaller sizes: the bytes (p + 85 c) mod 256 they hold)"""
    mean, std = norm
    src, _ = R.prep_src_f32(n, h, w, mean, std, 11)
    _prep_check(src, False, n, h, w, mean, std)
    _prep_check(R.prep_src_u8(n, h, w), True, n, h, w, mean, std)


@pytest.mark.parametrize('is_u8', [False, True], ids=['f32', 'u8'])
def test_prep_input_second_grid_trip(is_u8):
    n, h, w = 5, 456, 456
    assert n * (h + 8) * (w + 8) > R.GRID_CAP_ITEMS
    src = R.prep_src_u8(n, h, w) if is_u8 else R.prep_src_f32(n, h, w, R.IMAGENET_MEAN, R.IMAGENET_STD, 12)[0]
    _prep_check(src, is_u8, n, h, w, R.IMAGENET_MEAN, R.IMAGENET_STD)


# ------------------------------------------------------------------ max pool forward, bf16
def _pool_fwd(entry, x, n, h, w, c, with_arg=True, with_sign=True):
    """entry 'keep' or 'plain' -> pooled, codes, sign bytes (None where not asked for)"""
    L, lib = _lib()
    items = n * (h // 2) * (w // 2) * c
    out = _out(items)
    arg = _out(items, torch.uint8) if with_arg else None
    sign = _out(items // 8, torch.uint8) if with_sign and entry == 'keep' else None
    if entry == 'keep':
        L.check(lib.rart_engine_maxpool_keep(L.ptr(x), L.ptr(out), L.ptr(arg), L.ptr(sign), n, h, w, c, L.stream_ptr()))
    else:
        L.check(lib.rart_engine_maxpool(L.ptr(x), L.ptr(out), L.ptr(arg), n, h, w, c, L.stream_ptr()))
    assert _tail_ok(out, items) and (arg is None or _tail_ok(arg, items)) and (sign is None or _tail_ok(sign, items // 8))
    return tuple(t for t in (out[:items], None if arg is None else arg[:items], None if sign is None else sign[:items // 8]) if t is not None)


def _pool_want(x):
    """x NCHW on the CPU -> the flat NHWC expectations: pooled in the dtype of x, codes, sign bytes"""
    pooled, codes, sign = R.maxpool_ref(x)
    return R.nhwc(pooled).view(-1), R.nhwc(codes).view(-1), sign.view(-1)


def _pool_fwd_check(x, n, h, w, c):
    pooled, codes, sign = _pool_want(x)
    want = _bits(pooled.to(torch.bfloat16))
    dev = R.nhwc(x).to(torch.bfloat16).cuda()
    got, arg, sg = _twice(lambda: _pool_fwd('keep', dev, n, h, w, c))
    assert torch.equal(_bits(got).cpu(), want), 'pooled bits'
    assert torch.equal(arg.cpu(), codes), 'argmax codes'
    assert torch.equal(sg.cpu(), sign), 'sign bytes'
    # null argmax_out / sign_out: the other outputs are the same, and rart_engine_maxpool is the same pool without the sign bytes
    for entry, with_arg, with_sign in (('keep', True, False), ('keep', False, True), ('keep', False, False), ('plain', True, False),
                                       ('plain', False, False)):
        res = list(_pool_fwd(entry, dev, n, h, w, c, with_arg, with_sign))
        assert torch.equal(_bits(res.pop(0)), _bits(got))
        if with_arg:
            assert torch.equal(res.pop(0), arg)
        if with_sign:
            assert torch.equal(res.pop(0), sg)
    return dev, arg


@pytest.mark.parametrize('shape', R.POOL_SHAPES, ids=str)
@pytest.mark.parametrize('kind', ['lattice', 'relu'])
def test_maxpool_forward_bit_exact(kind, shape):
    n, h, w, c = shape
    _pool_fwd_check(R.pool_case(kind, shape), n, h, w, c)


def test_maxpool_forward_second_grid_trip():
    n, h, w, c = 17, 64, 64, 512
    assert n * (h // 2) * (w // 2) * (c // 8) > R.GRID_CAP_ITEMS
    x = R.lattice_pool_input_large(n, h, w, c, 21)
    pooled, codes, sign = _pool_want(x)
    dev = R.nhwc(x).to(torch.bfloat16).cuda()
    got, arg, sg = _twice(lambda: _pool_fwd('keep', dev, n, h, w, c))
    assert torch.equal(_bits(got).cpu(), _bits(pooled.to(torch.bfloat16)))
    assert torch.equal(arg.cpu(), codes) and torch.equal(sg.cpu(), sign)


# ------------------------------------------------------------------ max pool backward, bf16
def _pool_bwd(y, arg, dpool, n, h, w, c):
    L, lib = _lib()
    items = n * h * w * c
    dz = _out(items)
    L.check(lib.rart_engine_maxpool_bwd(L.ptr(y), L.ptr(arg), L.ptr(dpool), L.ptr(dz), n, h, w, c, L.stream_ptr()))
    assert _tail_ok(dz, items)
    return (dz[:items],)


@pytest.mark.parametrize('shape', R.POOL_SHAPES, ids=str)
@pytest.mark.parametrize('kind', ['lattice', 'relu'])
def test_maxpool_backward(kind, shape):
    """the kernel's own codes from the forward; lattice gradients bit-exact, randn gradients within the bound"""
    n, h, w, c = shape
    x = R.pool_case(kind, shape)
    dev, arg = _pool_fwd_check(x, n, h, w, c)
    codes = R.maxpool_ref(x)[1]
    pshape = (n, c, h // 2, w // 2)
    dead = (R.nhwc(x) <= 0).view(-1)
    assert dead.any() and not dead.all()
    # lattice gradients: the fp64 sum, cast to bf16 (it rounds nothing: |k| <= 256)
    dpool = R.lattice_grad_bf16(pshape, 31)
    want = R.nhwc(R.maxpool_bwd_ref(x, dpool)).view(-1)
    dz, = _twice(lambda: _pool_bwd(dev, arg, R.nhwc(dpool).to(torch.bfloat16).cuda(), n, h, w, c))
    dz = dz.cpu()
    assert torch.equal(_bits(dz), _bits(want.to(torch.bfloat16))), 'lattice gradient'
    assert (_bits(dz)[dead] == 0).all()                                   # +0 bits wherever y is +0, -0 or negative
    assert dz.double().sum().item() == dpool[codes != 15].sum().item()    # nothing lost, nothing counted twice
    # randn gradients
    g = torch.randn(pshape, generator=torch.Generator().manual_seed(32)).to(torch.bfloat16).double()
    want = R.nhwc(R.maxpool_bwd_ref(x, g)).view(-1)
    mag = R.nhwc(R.maxpool_bwd_ref(x, g.abs())).view(-1)
    dz, = _twice(lambda: _pool_bwd(dev, arg, R.nhwc(g).to(torch.bfloat16).cuda(), n, h, w, c))
    dz = dz.cpu()
    assert torch.isfinite(dz).all() and (_bits(dz)[dead] == 0).all()
    live = mag > 0
    ratio = ((dz.double() - want).abs()[live] / (_ulp_bf16(want) + 3 * U32 * mag)[live]).max().item()
    print('maxpool_bwd %s %s: worst |err| / (ulp + 3 U sum|terms|) = %.4f' % (kind, shape, ratio))
    assert ratio <= 1.0 and (_bits(dz)[~live] == 0).all()


def test_maxpool_backward_mask_alone():
    """hand-made codes: every window points at its centre (code 4), and y is +0, -0 or negative at a third of the centres"""
    n, h, w, c = 2, 6, 10, 16
    g = torch.Generator().manual_seed(41)
    y = torch.rand(n, c, h, w, generator=g).double() + 0.5
    cen = y[:, :, 0::2, 0::2]
    pick = torch.randint(0, 9, cen.shape, generator=g)
    for k, v in enumerate((0.0, -0.0, -1.5)):
        cen[pick == k] = v                                                # a view: writes y
    y[:, :, 1::2, 1::2] = -2.0                                            # and pixels no window names
    dpool = R.lattice_grad_bf16((n, c, h // 2, w // 2), 42)
    want = torch.zeros_like(y)
    want[:, :, 0::2, 0::2] = torch.where(cen > 0, dpool, torch.zeros_like(dpool))
    masked = (cen <= 0).double().mean().item()
    assert 0.25 <= masked <= 0.45
    arg = torch.full((n * (h // 2) * (w // 2) * c,), 4, dtype=torch.uint8, device='cuda')
    yd, dp = R.nhwc(y).to(torch.bfloat16).cuda(), R.nhwc(dpool).to(torch.bfloat16).cuda()
    dz, = _twice(lambda: _pool_bwd(yd, arg, dp, n, h, w, c))
    assert torch.equal(_bits(dz).cpu(), _bits(R.nhwc(want).to(torch.bfloat16)).view(-1))


def test_maxpool_backward_second_grid_trip():
    n, h, w, c = 5, 64, 64, 512
    assert n * h * w * (c // 8) > R.GRID_CAP_ITEMS
    x = R.lattice_pool_input_large(n, h, w, c, 22)
    dpool = R.lattice_grad_bf16((n, c, h // 2, w // 2), 23, torch.float32)
    dev = R.nhwc(x).to(torch.bfloat16).cuda()
    _, arg, _ = _pool_fwd('keep', dev, n, h, w, c)
    assert torch.equal(arg.cpu(), _pool_want(x)[1])
    want = R.nhwc(R.maxpool_bwd_ref(x, dpool)).view(-1)
    dz, = _twice(lambda: _pool_bwd(dev, arg, R.nhwc(dpool).to(torch.bfloat16).cuda(), n, h, w, c))
    assert torch.equal(_bits(dz).cpu(), _bits(want.to(torch.bfloat16)))


# ------------------------------------------------------------------ max pool on pairs
def _pool_fwd_pair(buf, lo_off, n, h, w, c, gap, with_arg=True, with_sign=True):
    L, lib = _lib()
    items = n * (h // 2) * (w // 2) * c
    out, out_lo = _pair_out(items, gap)
    arg = _out(items, torch.uint8) if with_arg else None
    sign = _out(items // 8, torch.uint8) if with_sign else None
    L.check(lib.rart_engine_maxpool_pair(L.ptr(buf), lo_off, L.ptr(out), out_lo, L.ptr(arg), L.ptr(sign), n, h, w, c, L.stream_ptr()))
    hi, lo = _pair_planes(out, items, gap)
    assert (arg is None or _tail_ok(arg, items)) and (sign is None or _tail_ok(sign, items // 8))
    return tuple(t for t in (hi, lo, None if arg is None else arg[:items], None if sign is None else sign[:items // 8]) if t is not None)


def _pool_pair_want(x):
    """x: fp32 NCHW of canonical pair values -> the input planes at the reference argmax (NHWC, flat), codes, sign bytes"""
    pooled, idx = R.maxpool_argmax(x.double() if x.numel() < 1 << 22 else x)
    planes = R.split(x)
    at = [R.nhwc(_bits(p).flatten(2).gather(2, idx.flatten(2)).view(idx.shape)).view(-1) for p in planes]          # bit patterns
    return at, R.nhwc(R.codes_from_index(idx, pooled, x.shape[3])).view(-1), R.pack_sign(pooled > 0).view(-1), planes


def _pool_pair_check(x, n, h, w, c, gaps):
    at, codes, sign, planes = _pool_pair_want(x)
    planes = [R.nhwc(p) for p in planes]
    arg = None
    for gap in gaps:
        buf, lo_off = _pair_in(planes, gap)
        hi, lo, arg, sg = _twice(lambda: _pool_fwd_pair(buf, lo_off, n, h, w, c, gap))
        assert torch.equal(_bits(hi).cpu(), at[0]) and torch.equal(_bits(lo).cpu(), at[1]), 'the input pair at the argmax'
        assert torch.equal(arg.cpu(), codes), 'argmax codes'
        assert torch.equal(sg.cpu(), sign), 'sign bytes'
    return arg


@pytest.mark.parametrize('shape', R.POOL_SHAPES, ids=str)
@pytest.mark.parametrize('kind', ['lattice_pair', 'relu_pair'])
def test_maxpool_pair_forward_bit_exact(kind, shape):
    """the lo plane directly behind hi, and numel + 64 elements behind it with NaN between; null argmax_out / sign_out"""
    n, h, w, c = shape
    x = R.pool_case(kind, shape)
    arg = _pool_pair_check(x, n, h, w, c, (0, TAIL))
    buf, lo_off = _pair_in([R.nhwc(p) for p in R.split(x)], 0)
    full = _pool_fwd_pair(buf, lo_off, n, h, w, c, 0)
    for with_arg, with_sign in ((True, False), (False, True), (False, False)):
        res = list(_pool_fwd_pair(buf, lo_off, n, h, w, c, 0, with_arg, with_sign))
        assert torch.equal(_bits(res.pop(0)), _bits(full[0])) and torch.equal(_bits(res.pop(0)), _bits(full[1]))
        if with_arg:
            assert torch.equal(res.pop(0), arg)
        if with_sign:
            assert torch.equal(res.pop(0), full[3])


def test_maxpool_pair_forward_second_grid_trip():
    n, h, w, c = 17, 64, 64, 512
    assert n * (h // 2) * (w // 2) * (c // 8) > R.GRID_CAP_ITEMS
    _pool_pair_check(R.lattice_pool_input_large(n, h, w, c, 24, pair=True), n, h, w, c, (0,))


def _pool_bwd_pair(arg, dp_buf, dp_lo, n, h, w, c, gap):
    L, lib = _lib()
    items = n * h * w * c
    dz, dz_lo = _pair_out(items, gap)
    L.check(lib.rart_engine_maxpool_bwd_pair(L.ptr(arg), L.ptr(dp_buf), dp_lo, L.ptr(dz), dz_lo, n, h, w, c, L.stream_ptr()))
    return _pair_planes(dz, items, gap)


def _pair_value(hi, lo):
    return hi.double().cpu() + lo.double().cpu()


@pytest.mark.parametrize('shape', R.POOL_SHAPES, ids=str)
@pytest.mark.parametrize('kind', ['lattice_pair', 'relu_pair'])
def test_maxpool_pair_backward(kind, shape):
    """the kernel's own codes; lattice gradients bit-exact (the fp64 sum cast to fp32 and split), randn gradients within the bound;
    both lo offsets"""
    n, h, w, c = shape
    x = R.pool_case(kind, shape)
    arg = _pool_pair_check(x, n, h, w, c, (0,))
    xd = x.double()
    codes = R.maxpool_ref(xd)[1]
    pshape = (n, c, h // 2, w // 2)
    dpool = R.lattice_grad_pair(pshape, 51)
    want64 = R.nhwc(R.maxpool_bwd_ref(xd, dpool)).view(-1)
    want = R.split(want64.float())
    assert torch.equal(want[0].double() + want[1].double(), want64)
    for gap in (0, TAIL):
        buf, lo_off = _pair_in(R.split(R.nhwc(dpool).float()), gap)
        hi, lo = _twice(lambda: _pool_bwd_pair(arg, buf, lo_off, n, h, w, c, gap))
        assert torch.equal(_bits(hi).cpu(), _bits(want[0])) and torch.equal(_bits(lo).cpu(), _bits(want[1])), 'lattice gradient'
        assert _pair_value(hi, lo).sum().item() == dpool[codes != 15].sum().item()
    g = R.split(torch.randn(pshape, generator=torch.Generator().manual_seed(52)))
    gv = g[0].double() + g[1].double()
    want = R.nhwc(R.maxpool_bwd_ref(xd, gv)).view(-1)
    mag = R.nhwc(R.maxpool_bwd_ref(xd, gv.abs())).view(-1)
    buf, lo_off = _pair_in([R.nhwc(p) for p in g], TAIL)
    hi, lo = _twice(lambda: _pool_bwd_pair(arg, buf, lo_off, n, h, w, c, TAIL))
    got = _pair_value(hi, lo)
    live = mag > 0
    assert torch.isfinite(got).all() and (_bits(hi).cpu()[~live] == 0).all() and (_bits(lo).cpu()[~live] == 0).all()
    ratio = ((got - want).abs()[live] / (2.0 ** -16 * want.abs() + 3 * U32 * mag)[live]).max().item()
    print('maxpool_bwd_pair %s %s: worst |err| / (2^-16 |ref| + 3 U sum|terms|) = %.4f' % (kind, shape, ratio))
    assert ratio <= 1.0


def test_maxpool_pair_backward_codes_alone():
    """hand-made codes: the centre (code 4) or 15; there is no y to read, the codes alone decide"""
    n, h, w, c = 2, 6, 10, 16
    g = torch.Generator().manual_seed(43)
    pshape = (n, c, h // 2, w // 2)
    codes = torch.where(torch.rand(pshape, generator=g) < 1 / 3, 15, 4).to(torch.uint8)
    dpool = R.lattice_grad_pair(pshape, 44)
    want64 = torch.zeros(n, c, h, w, dtype=torch.float64)
    want64[:, :, 0::2, 0::2] = torch.where(codes == 4, dpool, torch.zeros_like(dpool))
    want = R.split(R.nhwc(want64).float().view(-1))
    buf, lo_off = _pair_in(R.split(R.nhwc(dpool).float()), TAIL)
    arg = R.nhwc(codes).cuda()
    hi, lo = _twice(lambda: _pool_bwd_pair(arg, buf, lo_off, n, h, w, c, 0))
    assert torch.equal(_bits(hi).cpu(), _bits(want[0])) and torch.equal(_bits(lo).cpu(), _bits(want[1]))


def test_maxpool_pair_backward_second_grid_trip():
    n, h, w, c = 5, 64, 64, 512
    assert n * h * w * (c // 8) > R.GRID_CAP_ITEMS
    x = R.lattice_pool_input_large(n, h, w, c, 25, pair=True)
    dpool = R.lattice_grad_pair((n, c, h // 2, w // 2), 26, torch.float32)
    codes = R.nhwc(R.maxpool_ref(x)[1]).cuda()
    want = R.split(R.nhwc(R.maxpool_bwd_ref(x, dpool)).view(-1))
    buf, lo_off = _pair_in(R.split(R.nhwc(dpool)), 0)
    hi, lo = _twice(lambda: _pool_bwd_pair(codes, buf, lo_off, n, h, w, c, 0))
    assert torch.equal(_bits(hi).cpu(), _bits(want[0])) and torch.equal(_bits(lo).cpu(), _bits(want[1]))


def test_pair_pools_refuse_a_bad_lo_offset():
    """lo_off 0, negative, or not a multiple of 8: status nonzero, nothing written"""
    L, lib = _lib()
    n, h, w, c = 1, 4, 4, 8
    x, _ = _pair_in(R.split(torch.rand(n, h, w, c)), TAIL)
    dp, _ = _pair_in(R.split(torch.rand(n, h // 2, w // 2, c)), TAIL)
    codes = torch.full((n * (h // 2) * (w // 2) * c,), 4, dtype=torch.uint8, device='cuda')
    pooled_n, in_n = n * (h // 2) * (w // 2) * c, n * h * w * c
    for bad in (0, -8, in_n + 4, 12):
        for which in (0, 1):                                              # the input's offset, the output's
            out, out_lo = _pair_out(pooled_n, TAIL)
            arg, sign = _out(pooled_n, torch.uint8), _out(pooled_n // 8, torch.uint8)
            offs = (bad, out_lo) if which == 0 else (in_n + TAIL, bad)
            st = lib.rart_engine_maxpool_pair(L.ptr(x), offs[0], L.ptr(out), offs[1], L.ptr(arg), L.ptr(sign), n, h, w, c, L.stream_ptr())
            torch.cuda.synchronize()
            assert st != 0 and _pair_untouched(out, pooled_n, TAIL) and _untouched(arg, pooled_n) and _untouched(sign, pooled_n // 8), (bad, which)
            dz, dz_lo = _pair_out(in_n, TAIL)
            offs = (bad, dz_lo) if which == 0 else (pooled_n + TAIL, bad)
            st = lib.rart_engine_maxpool_bwd_pair(L.ptr(codes), L.ptr(dp), offs[0], L.ptr(dz), offs[1], n, h, w, c, L.stream_ptr())
            torch.cuda.synchronize()
            assert st != 0 and _pair_untouched(dz, in_n, TAIL), (bad, which)


# ------------------------------------------------------------------ col2im
C2I_SHAPES = [(1, 16, 32), (2, 32, 64), (1, 48, 32)]          # one tile with all four image edges; 2 x 2 tiles; three tiles in a column


def _col2im(f32, patches, n, h, w, std, cols=R.PATCH_COLS):
    L, lib = _lib()
    numel = n * 3 * h * w
    grad = _out(numel, torch.float32)
    fn = lib.rart_engine_stem_col2im_f32 if f32 else lib.rart_engine_stem_col2im
    st = fn(L.ptr(patches), L.ptr(grad), n, h, w, cols, _c3(std), L.stream_ptr())
    return st, grad, numel


def _col2im_ok(f32, patches, n, h, w, std):
    L, _ = _lib()
    st, grad, numel = _col2im(f32, patches, n, h, w, std)
    L.check(st)
    assert _tail_ok(grad, numel)
    return (grad[:numel].view(n, 3, h, w),)


def _patch_buf(values, f32):
    """values fp64 [n][h/2][w/2][147] -> device patches [..][152] of the kernel's type, NaN in columns 147..151"""
    buf = torch.full(values.shape[:3] + (R.PATCH_COLS,), NAN, dtype=torch.float32 if f32 else torch.bfloat16)
    buf[..., :147] = values
    assert torch.equal(buf[..., :147].double(), values)
    return buf.cuda()


@pytest.mark.parametrize('norm', NORMS, ids=NORM_IDS)
@pytest.mark.parametrize('n,h,w', C2I_SHAPES)
@pytest.mark.parametrize('f32', [False, True], ids=['bf16', 'f32'])
def test_col2im_lattice_and_randn(f32, n, h, w, norm):
    std = norm[1]
    shape = (n, h // 2, w // 2, 147)
    lattice = (R.lattice_grad_pair if f32 else R.lattice_grad_bf16)(shape, 61)
    got, = _twice(lambda: _col2im_ok(f32, _patch_buf(lattice, f32), n, h, w, std))
    assert torch.equal(got.cpu().view(torch.int32), R.col2im_ref(lattice, std).view(torch.int32)), 'lattice patches'
    rnd = torch.randn(shape, generator=torch.Generator().manual_seed(62))
    rnd = (rnd if f32 else rnd.to(torch.bfloat16)).double()
    got, = _twice(lambda: _col2im_ok(f32, _patch_buf(rnd, f32), n, h, w, std))
    istd = R.istd32(std).double().view(1, 3, 1, 1)
    s64, mag = R.col2im_sum64(rnd), R.col2im_sum64(rnd.abs())
    assert torch.isfinite(got).all()
    ratio = ((got.cpu().double() - istd * s64).abs() / (istd * (16 * U32 * mag + U32 * s64.abs()))).max().item()
    print('col2im %s %s std %s: worst |err| / bound = %.4f' % ('f32' if f32 else 'bf16', (n, h, w), 'imagenet' if std else 'none', ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize('f32', [False, True], ids=['bf16', 'f32'])
def test_col2im_one_hot_sweep(f32):
    """a single nonzero entry at each of the 147 columns (image j of the batch holds column j, value j + 1) of one patch: at the four
    corners, on an image edge, and on either side of the tile boundaries (pixel rows 15 | 16, pixel columns 31 | 32 at 32 x 64).  It
    lands on exactly one pixel, or on none where the tap lies outside the image."""
    h, w, n = 32, 64, 147
    patches = torch.zeros(n, h // 2, w // 2, R.PATCH_COLS, dtype=torch.float32 if f32 else torch.bfloat16, device='cuda')
    patches[..., 147:] = NAN
    cols = torch.arange(147, device='cuda')
    hits = 0
    for std in (None, R.IMAGENET_STD):
        istd = R.istd32(std)
        for p, q in ((0, 0), (0, 31), (15, 0), (15, 31), (0, 10), (9, 31), (7, 15), (8, 16), (7, 16), (8, 15)):
            patches[cols, p, q, cols] = (cols + 1).to(patches.dtype)
            want = torch.zeros(n, 3, h, w)
            for col in range(147):
                t = R.one_hot_target(p, q, col, h, w)
                if t is not None:
                    want[col, t[0], t[1], t[2]] = torch.tensor(col + 1.0) * istd[t[0]]
                    hits += 1
            got, = _col2im_ok(f32, patches, n, h, w, std)
            assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), (p, q)
            patches[cols, p, q, cols] = 0
    assert hits > 2 * 10 * 147 // 2


@pytest.mark.parametrize('f32', [False, True], ids=['bf16', 'f32'])
def test_col2im_refuses_what_its_header_forbids(f32):
    patches = torch.zeros(1, 16, 32, R.PATCH_COLS, dtype=torch.float32 if f32 else torch.bfloat16, device='cuda')
    for h, w, cols in ((8, 32, 152), (16, 16, 152), (16, 32, 147)):
        st, grad, numel = _col2im(f32, patches, 1, h, w, None, cols)
        torch.cuda.synchronize()
        assert st != 0 and _untouched(grad, numel), (h, w, cols)
