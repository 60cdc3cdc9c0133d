"""Plain torch / numpy references and input generators for the stem glue kernels of the ResNet-50 engines (csrc/engine_aux.hip,
both storages): input preparation, the 3x3/2 max pool with its argmax codes and sign bits, its backward, and the stem's
col2im.  Nothing of the library is imported here.  tests/test_stem_glue_refs_cpu.py pins these functions and the properties of the
generated inputs without a GPU; tests/test_stem_glue_kernels_gpu.py holds the kernels to them.

Layouts: the references take and return NCHW (torch's), the kernels work on NHWC: nhwc() converts.  Codes are one byte per
(window, channel): the window position ky * 3 + kx of the first maximum in scan order, or 15 where the pooled value is not > 0.
Sign bits: uint8 [n][h/2][w/2][c/8], bit j of byte k = (pooled channel 8k + j > 0)."""
import numpy as np
import torch
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
GRID_CAP_ITEMS = 256 * 16 * 256                     # grid_for: at most 256 * 16 workgroups of 256 threads; more items take a second trip


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def split(t):
    """fp32 -> the pair of bf16 planes [2][...]: hi = bf16_rne(v), lo = bf16_rne(v - hi)"""
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


def canonical(v):
    """fp32 values v with split(v)[0] + split(v)[1] == v and a split that is stable under re-splitting"""
    v = v.float()
    for _ in range(4):
        p = split(v)
        nxt = p[0].float() + p[1].float()
        if torch.equal(nxt, v):
            break
        v = nxt
    return v


# ------------------------------------------------------------------ input preparation
def _norm32(mean, std):
    mean32 = np.zeros(3, np.float32) if mean is None else np.asarray(mean, dtype=np.float32)
    istd32 = np.ones(3, np.float32) if std is None else np.float32(1) / np.asarray(std, dtype=np.float32)
    return mean32, istd32


def prep_x01(src, is_u8):
    """the fp32 [0, 1] image as NHWC [n][h][w][3]: the fp32 source itself (NCHW), or float32(byte) * (float32(1) / float32(255))"""
    if is_u8:
        assert src.dtype == torch.uint8 and src.shape[-1] == 3
        return src.float() * torch.tensor(np.float32(1) / np.float32(255))
    assert src.dtype == torch.float32 and src.shape[1] == 3
    return nhwc(src)


def prep_ref(src, is_u8, mean, std):
    """k_prep_input op by op in fp32 (torch's CPU elementwise ops round every operation, nothing is contracted):
    v = (x - mean) * istd, hi = bf16_rne(v), lo = bf16_rne(v - hi) -> hi, lo bf16 [n][h+8][w+8][4], the image at (3, 3), +0 elsewhere"""
    mean32, istd32 = _norm32(mean, std)
    x = prep_x01(src, is_u8)
    n, h, w, _ = x.shape
    v = (x - torch.from_numpy(mean32)) * torch.from_numpy(istd32)
    assert v.dtype == torch.float32
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    out = torch.zeros(2, n, h + 8, w + 8, 4, dtype=torch.bfloat16)
    out[0, :, 3:3 + h, 3:3 + w, :3] = hi
    out[1, :, 3:3 + h, 3:3 + w, :3] = lo
    return out[0], out[1]


def prep_v64(src, is_u8, mean, std):
    """(x - mean) / std in fp64 of the fp32 operands (x the fp32 [0, 1] value, mean and std as fp32), NHWC"""
    mean32 = np.zeros(3, np.float32) if mean is None else np.asarray(mean, dtype=np.float32)
    std32 = np.ones(3, np.float32) if std is None else np.asarray(std, dtype=np.float32)
    return (prep_x01(src, is_u8).double() - torch.from_numpy(mean32).double()) / torch.from_numpy(std32).double()


def prep_boundary_values(mean_c, std_c, count=20):
    """fp32 x in [0, 1] whose v = (x - mean) / std lies within an fp32 ulp or two of a bf16 rounding boundary (the midpoint of two
    neighbouring bf16 values), on either side of it: the fp32 nearest to the boundary's preimage and its two neighbours"""
    mean64 = float(np.float32(0 if mean_c is None else mean_c))
    std64 = float(np.float32(1 if std_c is None else std_c))
    lo_v, hi_v = (0.0 - mean64) / std64, (1.0 - mean64) / std64
    hs = torch.linspace(lo_v * 0.95 + 0.01, hi_v * 0.95, count).to(torch.bfloat16).float().numpy()       # bf16 values inside the range
    out = []
    for hv in hs:
        bits = np.array([hv], np.float32).view(np.uint32)
        mid = float((bits | np.uint32(0x8000)).view(np.float32)[0])          # half a bf16 ulp further from zero: exact in fp32
        x = np.float32(mid * std64 + mean64)
        for cand in (np.nextafter(x, np.float32(-1)), x, np.nextafter(x, np.float32(2))):
            if 0.0 <= cand <= 1.0:
                out.append(cand)
    return np.array(out, np.float32)


def prep_src_f32(n, h, w, mean, std, seed):
    """fp32 NCHW in [0, 1]: random, and from pixel 0 of every channel on mean[c] itself, 0, 1 and prep_boundary_values (as many
    as fit)"""
    g = torch.Generator().manual_seed(seed)
    src = torch.rand(n, 3, h, w, generator=g)
    flat = src.permute(1, 0, 2, 3).reshape(3, -1).clone()
    planted = []
    for c in range(3):
        mc = None if mean is None else mean[c]
        special = np.concatenate([np.array([0.0 if mc is None else mc, 0.0, 1.0], np.float32),
                                  prep_boundary_values(mc, None if std is None else std[c])])
        k = min(len(special), flat.shape[1])
        flat[c, :k] = torch.from_numpy(special[:k])
        planted.append(k)
    return flat.reshape(3, n, h, w).permute(1, 0, 2, 3).contiguous(), planted


def prep_src_u8(n, h, w):
    """uint8 NHWC: pixel p of channel c holds byte (p + 85 c) mod 256, so every channel sees every byte once n h w >= 256"""
    p = torch.arange(n * h * w, dtype=torch.int64).view(n, h, w, 1)
    return ((p + 85 * torch.arange(3, dtype=torch.int64)) % 256).to(torch.uint8)


# ------------------------------------------------------------------ max pool
def maxpool_argmax(x):
    """F.max_pool2d(x, 3, 2, 1) on the CPU -> pooled [n][c][h/2][w/2] and the flat index iy * w + ix of each window's maximum"""
    assert x.device.type == 'cpu' and x.is_contiguous()
    return F.max_pool2d(x, 3, 2, 1, return_indices=True)


def codes_from_index(idx, pooled, w):
    oh, ow = idx.shape[2], idx.shape[3]
    oy = torch.arange(oh).view(1, 1, oh, 1)
    ox = torch.arange(ow).view(1, 1, 1, ow)
    code = (idx // w - (2 * oy - 1)) * 3 + (idx % w - (2 * ox - 1))
    assert int(code.min()) >= 0 and int(code.max()) <= 8
    return torch.where(pooled > 0, code, torch.full_like(code, 15)).to(torch.uint8)


def pack_sign(pos):
    """pos: bool [n][c][oh][ow] -> uint8 [n][oh][ow][c/8], bit j of byte k = channel 8k + j"""
    n, c, oh, ow = pos.shape
    bits = nhwc(pos).view(n, oh, ow, c // 8, 8).to(torch.int32) * (2 ** torch.arange(8, dtype=torch.int32))
    return bits.sum(-1).to(torch.uint8)


def maxpool_ref(x):
    """x: NCHW (fp64; fp32 for the large cases) on the CPU -> pooled NCHW, codes uint8 NCHW, sign bytes [n][h/2][w/2][c/8]"""
    pooled, idx = maxpool_argmax(x)
    return pooled, codes_from_index(idx, pooled, x.shape[3]), pack_sign(pooled > 0)


def maxpool_bwd_ref(x, dpool):
    """autograd of that pool, times (x > 0): NCHW, the dtype of x"""
    xr = x.detach().clone().requires_grad_(True)
    pooled = F.max_pool2d(xr, 3, 2, 1)
    dz, = torch.autograd.grad(pooled, xr, dpool.to(x.dtype))
    return torch.where(x > 0, dz, torch.zeros_like(dz))


def window_codes(x, rule='first'):
    """The codes from the unfolded windows, without max_pool2d: the first (PyTorch's, the kernels') or the last maximum in scan order.
    `last` is what a kernel that compares with >= records; the generators are asserted to tell the two apart."""
    n, c, h, w = x.shape
    xp = F.pad(x, (1, 1, 1, 1), value=float('-inf'))
    win = xp.unfold(2, 3, 2).unfold(3, 3, 2)[:, :, :h // 2, :w // 2].reshape(n, c, h // 2, w // 2, 9)
    m = win.max(-1, keepdim=True).values
    pos = torch.arange(9).expand_as(win)
    eq = win == m
    code = torch.where(eq, pos, torch.full_like(pos, 9)).min(-1).values if rule == 'first' else \
        torch.where(eq, pos, torch.full_like(pos, -1)).max(-1).values
    return torch.where(m[..., 0] > 0, code, torch.full_like(code, 15)).to(torch.uint8)


def tied_share(x):
    """share of the windows whose maximum occurs more than once"""
    return (window_codes(x, 'first') != window_codes(x, 'last')).double().mean().item()


def window_class(oy, ox):
    """'corner', 'top', 'left' or 'interior': the pad cuts row 0 of the windows with oy = 0 and column 0 of those with ox = 0 (the sizes
    are even, so no window reaches past the bottom or the right edge)"""
    return 'corner' if oy == 0 and ox == 0 else 'top' if oy == 0 else 'left' if ox == 0 else 'interior'


def class_codes(cls):
    """the window positions that lie inside the image for a window of that class"""
    return [ky * 3 + kx for ky in range(3) for kx in range(3) if not (ky == 0 and cls in ('corner', 'top')) and
            not (kx == 0 and cls in ('corner', 'left'))]


def _plant(x, top, dead_values, negative_values, decoy=None):
    """Into the windows with even (oy, ox), which share no pixel with each other: round-robin per window class over the codes its
    geometry allows and 15.  Code t: `top` (above every drawn value) at position t and, for t < 8, again at position 8, so the window
    is tied and the first maximum is at t; `decoy` (pairs: a value below `top` with the same hi plane) goes to the window's first
    position when t is a later one, so that a comparison of the hi planes alone stops there.  Code 15: alternately every pixel of the window <= 0 with zeros of both signs, and every
    pixel strictly negative (the pooled value is then a negative number)."""
    n, c, h, w = x.shape
    count = {}
    for img in range(n):
        for ch in range(c):
            for oy in range(0, h // 2, 2):
                for ox in range(0, w // 2, 2):
                    cls = window_class(oy, ox)
                    allowed = class_codes(cls) + [15, 15]
                    k = count.get(cls, 0)
                    count[cls] = k + 1
                    t = allowed[k % len(allowed)]
                    if t == 15:
                        vals = dead_values if k % len(allowed) == len(allowed) - 1 else negative_values
                        for j, pos in enumerate(class_codes(cls)):
                            x[img, ch, 2 * oy - 1 + pos // 3, 2 * ox - 1 + pos % 3] = vals[(j + k) % len(vals)]
                    else:
                        first = class_codes(cls)[0]
                        if decoy is not None and t != first:
                            x[img, ch, 2 * oy - 1 + first // 3, 2 * ox - 1 + first % 3] = decoy
                        x[img, ch, 2 * oy - 1 + t // 3, 2 * ox - 1 + t % 3] = top
                        if t < 8:
                            x[img, ch, 2 * oy + 1, 2 * ox + 1] = top
    return x


def _signed_zeros(x, gen):
    """a third of the zeros become -0.0"""
    flip = (x == 0) & (torch.rand(x.shape, generator=gen) < 1 / 3)
    return torch.where(flip, torch.full_like(x, -0.0), x)


def lattice_pool_input(n, h, w, c, seed):
    """fp64 NCHW, exact in bf16: k / 4 with k in [-4, 8] (about three windows in ten have a tied maximum), zeros of both signs, and
    the planted windows of _plant"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 9, (n, c, h, w), generator=g).double() / 4
    x = _signed_zeros(x, g)
    return _plant(x, 2.25, [0.0, -0.0, -1.0, -0.25], [-1.0, -0.5, -0.25])


def lattice_pool_input_pair(n, h, w, c, seed):
    """fp32 NCHW of canonical pair values: six in ten are 1 + k 2^-12 with k in [0, 7] (the hi plane is 1.0 for all of them, so the
    lo plane decides, and exact duplicates are frequent), the rest k / 4 with k in [-4, 4]; planted as _plant.  Zeros are +0: a pair has
    no canonical -0 (split(-0) is (-0, +0), whose sum is +0)"""
    g = torch.Generator().manual_seed(seed)
    near_one = 1 + torch.randint(0, 8, (n, c, h, w), generator=g).double() * 2.0 ** -12
    coarse = torch.randint(-4, 5, (n, c, h, w), generator=g).double() / 4
    x = torch.where(torch.rand(n, c, h, w, generator=g) < 0.6, near_one, coarse)
    return _plant(x, 1.5 + 2.0 ** -10, [0.0, 0.0, -1.0 - 2.0 ** -12, -0.25], [-1.0, -1.0 - 2.0 ** -12, -0.25], decoy=1.5).float()


def relu_pool_input(n, h, w, c, seed, pair=False):
    """relu(randn) in bf16 (or as canonical pair values, fp32) with zeros of both signs (bf16 only) and the planted windows, which are not a ReLU
    output: all-negative windows whose pooled value is a negative number; fp64 NCHW (fp32 for pairs)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.relu(torch.randn(n, c, h, w, generator=g))
    v = canonical(v) if pair else v.to(torch.bfloat16).float()
    if pair:
        return _plant(v.double(), 16.0 + 2.0 ** -6, [0.0, 0.0, -1.0, -0.25], [-1.0, -0.5, -0.25], decoy=16.0).float()
    return _plant(_signed_zeros(v.double(), g), 16.0, [0.0, -0.0, -1.0, -0.25], [-1.0, -0.5, -0.25])


def lattice_pool_input_large(n, h, w, c, seed, pair=False):
    """the lattice alone, in fp32 and without planting (which loops): for the cases with more items than one launch holds"""
    g = torch.Generator().manual_seed(seed)
    if pair:
        k = torch.randint(-4, 8, (n, c, h, w), generator=g, dtype=torch.int32)
        return torch.where(k >= 0, 1 + k.float() * 2.0 ** -12, k.float() / 4)
    return torch.randint(-4, 9, (n, c, h, w), generator=g, dtype=torch.int32).float() / 4


# ------------------------------------------------------------------ gradients and patches
def lattice_grad_bf16(shape, seed, dtype=torch.float64):
    """multiples of 1/8 with |k| <= 64: exact in bf16, and every sum of <= 16 of them is exact in fp32 (and in bf16 for <= 4)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 65, shape, generator=g).to(dtype) / 8


def lattice_grad_pair(shape, seed, dtype=torch.float64):
    """k 2^-12 with |k| < 2^15: exact as a pair, every sum of <= 16 of them is exact in fp32, of <= 4 of them exact as a pair"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 15 + 1, 2 ** 15, shape, generator=g).to(dtype) * 2.0 ** -12


# ------------------------------------------------------------------ col2im
PATCH_COLS = 152                                     # 147 = 7 * 7 * 3 rounded up to 8; columns 147..151 are never read


def col2im_sum64(patches):
    """patches [n][h/2][w/2][>= 147] (column (r * 7 + s) * 3 + c) -> the fp64 sum NCHW [n][3][h][w]: F.fold, kernel 7, stride 2, pad 3"""
    n, oh, ow, _ = patches.shape
    p = patches[..., :147].double().reshape(n, oh * ow, 49, 3).permute(0, 3, 2, 1).reshape(n, 147, oh * ow)      # fold's c * 49 + r * 7 + s
    return F.fold(p, (2 * oh, 2 * ow), kernel_size=7, stride=2, padding=3)


def istd32(std):
    return torch.from_numpy(_norm32(None, std)[1])


def col2im_ref(patches, std):
    """the fp64 sum cast to fp32, times float32(1) / float32(std[c]) in fp32 -> fp32 NCHW"""
    return col2im_sum64(patches).float() * istd32(std).view(1, 3, 1, 1)


def one_hot_target(p, q, col, h, w):
    """the pixel (c, y, x) a patch entry lands on, or None where it falls outside the image"""
    r, s, c = col // 21, col // 3 % 7, col % 3
    y, x = 2 * p - 3 + r, 2 * q - 3 + s
    return (c, y, x) if 0 <= y < h and 0 <= x < w else None


# ------------------------------------------------------------------ the cases both test modules use
POOL_SHAPES = [(1, 2, 2, 8), (2, 2, 8, 8), (3, 6, 10, 64), (1, 16, 16, 24)]          # (n, h, w, c)
POOL_KINDS = ('lattice', 'relu', 'lattice_pair', 'relu_pair')
_pool_cache = {}


def pool_case(kind, shape):
    """the pool input of a case, NCHW on the CPU (fp64; fp32 canonical pair values for the pair kinds): drawn once, not to be written to"""
    key = (kind, shape)
    if key not in _pool_cache:
        n, h, w, c = shape
        seed = 1000 * h + 10 * w + c + n
        _pool_cache[key] = {'lattice': lambda: lattice_pool_input(n, h, w, c, seed),
                            'relu': lambda: relu_pool_input(n, h, w, c, seed),
                            'lattice_pair': lambda: lattice_pool_input_pair(n, h, w, c, seed),
                            'relu_pair': lambda: relu_pool_input(n, h, w, c, seed, pair=True)}[kind]()
    return _pool_cache[key]
