"""fp64 references, fp32 mirrors, input generators and bounds for the plain row kernels every engine calls through engine_base.py
(_rows, _ln, _ln_bwd, _fc1_gelu): rart_layernorm[_bwd]_{bf16,pair}, rart_softmax[_bwd]_rows_{bf16,pair} and rart_gelu[_bwd]_bf16
(LayerNorm: csrc/row_norm.hip; soft-max: csrc/vit_aux.hip, csrc/vit_bwd.hip, csrc/vit_pair.hip; GELU: csrc/vit_bwd.hip).  Nothing of
the library is imported here.
tests/test_row_kernel_refs_cpu.py shows without a GPU that a plain fp32 implementation meets every bound and that a list of wrong
implementations does not; tests/test_row_kernels_gpu.py holds the kernels to the bounds.

References: fp64, on the values the stored operands represent (bf16: the bf16 value; a pair: hi + lo).  LayerNorm and GELU come
from torch.nn.functional in fp64 and its autograd (the LayerNorm residual is added after autograd); the soft-max forward from
torch.softmax(scale * s); the soft-max backward is torch's own soft-max derivative (aten._softmax_backward_data, the function
autograd calls) applied to the STORED probabilities, times scale: the kernel is handed P, not the scores, and a rounded P is not
the soft-max of anything.  sm_bwd_ref_from_scores is the same derivative through autograd on the scores; the CPU test ties the two.

Mirrors: what each kernel's comment says it computes, in plain fp32 torch (two-pass biased variance with eps inside the root;
exp(s * scale - max) / sum; 0.5 v (1 + erf(v / sqrt 2)); Phi + v phi), with the output stored as the kernel stores it (bf16: one
rounding; pair: split()).  `variant` swaps in one deliberate mistake.  No GPU test compares against a mirror.

Bounds, per element, ref = the fp64 value, ulp = 2^-7 for a bf16 output and 2^-15 for a pair (one unit in the last place of the
stored result), 2e-5 / 3e-5 the thresholds the suite already gives the pair LayerNorm kernels, here per row instead of per tensor:
  LayerNorm forward    ulp |ref| + 2e-5 max_row(|gamma xhat| + |beta|) + MEAN_ROUNDINGS 2^-24 max_row|x| rstd |gamma|
  LayerNorm backward   ulp |ref| + 3e-5 (max_row|rstd dy gamma| + max_row|res|)
  soft-max forward     ulp ref + 1e-6
  soft-max backward    ulp |ref| + 1e-6 max_row|ref| + DOT_ROUNDINGS 2^-24 scale |P| sum_k |P_k dP_k|
  GELU                 2^-7 |ref| + 2^-23 |u|              (the fp32 rounding of 1 + erf, times u / 2: the negative tail)
  GELU'                |dh| (2^-7 |gelu'(u)| + 2^-22 (1 + min(|u|, 10)))
Two terms are not in the first statement of these bounds; the CPU test shows on the mirror why each is needed.
  * LayerNorm forward, third term: x - mean is taken against an fp32 mean, which one wave forms with 16 serial additions per lane,
    6 butterfly steps and a division (MEAN_ROUNDINGS = 23 roundings of at most 2^-24 max|x| each).  On the planted row (a)
    (mean 100, spread 0.05) held as a pair that is up to 23 * 6e-8 * 100 * 20 = 2.8e-3 of xhat, and the mirror measures 2.7
    times the first two terms there; on ordinary rows the term is a twentieth of the second one.  In bf16 row (a) rounds to the
    constant 100 (bf16's step at 100 is 0.5), so only the pair kernels see its spread.
  * soft-max backward, third term: the row's dot product is an fp32 number.  Where one probability is 1 - delta (the planted row
    with its maximum in column 0 at scale 1, and any 8 randn row one score dominates) dP - dot cancels to the size of delta in that
    column and every other column's value is of that size too, so neither relative term covers the 2^-24 |dot| the fp32 dot is
    off by: the mirror measures up to 3e4 times the first two terms.  DOT_ROUNDINGS counts what a wave spends on the dot: one for
    all the products together, one per addition in a lane (16 columns per lane in the bf16 kernels, 4 in the pair kernels) and 6
    butterfly steps, each at most 2^-24 sum|P dP|.  The count is needed, two roundings are not enough: sm_bwd_mirror(order='lanes')
    forms the dot in exactly that order with fused multiply-adds, and at (n_valid, ld) = (5, 8, 8), scale 1, it is at 1.135 of a
    2^-23 term (the first GPU run of rart_softmax_bwd_rows_pair measured the same 1.135, digit for digit)."""
import math

import torch
import torch.nn.functional as F

ULP = {'bf16': 2.0 ** -7, 'pair': 2.0 ** -15}
EPS = 1e-6                                           # the only value a caller passes (engine_base.py: _ln, _ln_bwd)
MEAN_ROUNDINGS = 23
DOT_ROUNDINGS = {'bf16': 1 + 16 + 6, 'pair': 1 + 4 + 6}
GRID_DEFAULT_ITEMS = 2048 * 256                      # csrc/rart_common.h: rart_grid_for's default, 256 * 8 workgroups of 256 threads
GELU_GRID_ITEMS = 256 * 16 * 256                     # csrc/vit_bwd.hip: grid_for passes 256 * 16 workgroups; more 8-element items take a second trip

LN_DIMS = (8, 16, 128, 256, 504, 512, 520, 768, 1016, 1024)      # one vector, parts of slot 0, slot 0, one vector into slot 1, ViT, one short, full
SLOT1_DIMS = (520, 768, 1016, 1024)
LN_SHAPES = [(r, d) for d in LN_DIMS for r in (6, 9)] + [(8, 128), (8, 768), (1, 768)]           # (rows, dim); rows = 1 has no planted rows
HEAD_SHAPE = (3, 5, 768)                             # (B, T, D) of the ViT head's layouts
ROW_A, ROW_B, ROW_C, ROW_D = 1, 2, 3, 4              # the planted rows; (e) is the last row
SM_SHAPES = {'bf16': [(1, 8, 8), (7, 8, 16), (8, 8, 8), (197, 200, 224), (512, 512, 512), (513, 520, 520), (1017, 1024, 1024),
                      (1024, 1024, 1024)],
             'pair': [(1, 4, 4), (3, 4, 8), (4, 4, 4), (5, 8, 8), (197, 200, 224), (252, 252, 256), (253, 256, 256), (256, 256, 256)]}
SM_ROWS_EXTRA = {'bf16': (9, (197, 200, 224)), 'pair': (9, (197, 200, 224))}                     # the one case with rows = 9
SM_SCALES = (0.125, 1.0)
SM_EQUAL, SM_ONE_HOT, SM_MAX_FIRST = 1, 2, 3         # the planted score rows
GELU_DH = (1.0, -0.37109375, 2.0 ** 14)
NAN = float('nan')


# ------------------------------------------------------------------ storage
def split(t):
    """fp32 -> the pair of bf16 planes [2][...]: hi = bf16_rne(v), lo = bf16_rne(v - hi) (the suite's _split)"""
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


def canonical(v):
    """fp32 values with split(v)[0] + split(v)[1] == v and a split that is stable under re-splitting"""
    v = v.float()
    for _ in range(4):
        p = split(v)
        nxt = p[0].float() + p[1].float()
        if torch.equal(nxt, v):
            break
        v = nxt
    return v


def store(v, prec):
    """fp32 -> the nearest values the storage holds, as fp32 (NaN stays NaN)"""
    return v.to(torch.bfloat16).float() if prec == 'bf16' else torch.where(torch.isnan(v), v, canonical(torch.nan_to_num(v)))


def planes(v, prec):
    """fp32 values -> the bf16 planes the storage holds: [v] or [hi, lo]; also the stored form of an fp32 result"""
    return [v.to(torch.bfloat16)] if prec == 'bf16' else list(split(v))


def value64(pl):
    return sum(p.double() for p in pl)


def stored64(r32, prec):
    """an fp32 result as the kernel stores it, read back in fp64"""
    return value64(planes(r32, prec))


def worst(err, bound):
    """max |err| / bound; a non-finite error, or any error against a zero bound, counts as infinite"""
    err, bound = err.double().abs().reshape(-1), bound.double().reshape(-1)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float('inf')))
    return r.max().item()


def worst_per_row(err, bound):
    return [worst(err[i], bound[i]) for i in range(err.shape[0])]


# ------------------------------------------------------------------ LayerNorm
def rows_for(rows, dim, gen, planted=True):
    """fp32 [rows][dim]: 2 randn + 0.3 (the rows the existing tests use) and, when planted (rows >= 6), at fixed indices
    (a) 100 + 0.05 randn: large mean, small spread; (b) the constant 3.25: variance exactly 0; (c) zeros with 50 in the last
    column, the last lane of the last occupied vector slot; (d) 1e-3 randn: variance comparable with eps; (e) a copy of row 0 at
    the last index."""
    x = 2 * torch.randn(rows, dim, generator=gen) + 0.3
    if planted:
        assert rows >= 6
        x[ROW_A] = 100 + 0.05 * torch.randn(dim, generator=gen)
        x[ROW_B] = 3.25
        x[ROW_C] = 0
        x[ROW_C, dim - 1] = 50
        x[ROW_D] = 1e-3 * torch.randn(dim, generator=gen)
        x[rows - 1] = x[0]
    return x


_ln_cache = {}


def ln_case(rows, dim, prec):
    """the operands of a LayerNorm case as stored fp32 values on the CPU: x, dy, res [rows][dim], gamma = 1 + 0.1 randn,
    beta = randn (fp32 parameters).  dy and res repeat row 0 at the last index like x.  Drawn once: not to be written to."""
    key = (rows, dim, prec)
    if key not in _ln_cache:
        g = torch.Generator().manual_seed(100000 + 1000 * rows + dim)
        planted = rows >= 6
        x = store(rows_for(rows, dim, g, planted), prec)
        dy, res = store(torch.randn(rows, dim, generator=g), prec), store(torch.randn(rows, dim, generator=g), prec)
        if planted:
            dy[rows - 1], res[rows - 1] = dy[0], res[0]
        _ln_cache[key] = dict(x=x, dy=dy, res=res, gamma=1 + 0.1 * torch.randn(dim, generator=g), beta=torch.randn(dim, generator=g),
                              planted=planted)
    return _ln_cache[key]


def _ln64(x, gamma, beta, eps):
    xr = x.double().requires_grad_(True)
    return xr, F.layer_norm(xr, (x.shape[-1],), gamma.double(), beta.double(), eps)


def _stats64(x, eps):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean) ** 2).mean(-1, keepdim=True).add(eps).rsqrt()
    return (x - mean) * rstd, rstd


def ln_fwd_ref(x, gamma, beta, eps=EPS):
    return _ln64(x, gamma, beta, eps)[1].detach()


def ln_fwd_bound(x, gamma, beta, prec, eps=EPS):
    ref = ln_fwd_ref(x, gamma, beta, eps)
    xhat, rstd = _stats64(x, eps)
    row = ((gamma.double() * xhat).abs() + beta.double().abs()).amax(-1, keepdim=True)
    mean_term = MEAN_ROUNDINGS * 2.0 ** -24 * x.double().abs().amax(-1, keepdim=True) * rstd * gamma.double().abs()
    return ULP[prec] * ref.abs() + 2e-5 * row + mean_term, ULP[prec] * ref.abs() + 2e-5 * row


def ln_bwd_ref(x, dy, gamma, res=None, eps=EPS):
    """autograd of the fp64 layer_norm (beta does not enter), the residual added afterwards"""
    xr, y = _ln64(x, gamma, torch.zeros_like(gamma), eps)
    gx, = torch.autograd.grad(y, xr, grad_outputs=dy.double())
    return gx if res is None else gx + res.double()


def ln_bwd_bound(x, dy, gamma, res, prec, eps=EPS):
    ref = ln_bwd_ref(x, dy, gamma, res, eps)
    _, rstd = _stats64(x, eps)
    row = (rstd * dy.double() * gamma.double()).abs().amax(-1, keepdim=True)
    if res is not None:
        row = row + res.double().abs().amax(-1, keepdim=True)
    return ULP[prec] * ref.abs() + 3e-5 * row


def _ln_stats32(x, eps, variant):
    """mean and rstd [rows][1] in fp32, as the kernels form them; variant: one deliberate mistake"""
    d = x.shape[-1]
    keep = torch.ones(d, dtype=torch.bool)
    if variant == 'skip_slot1':
        keep[512:] = False                           # lane l's second vector, l + 64: columns from 512 on
    if variant == 'skip_last_vector':
        keep[d - 8:] = False
    xs = torch.where(keep, x, torch.zeros_like(x))
    mean = xs.sum(-1, keepdim=True) / d
    if variant == 'one_pass':
        var = (xs * xs).sum(-1, keepdim=True) / d - mean * mean
    else:
        t = torch.where(keep, x - mean, torch.zeros_like(x))
        var = (t * t).sum(-1, keepdim=True) / (d - 1 if variant == 'unbiased' else d)
    eps32 = torch.tensor(eps, dtype=torch.float32)
    rstd = 1.0 / (var.sqrt() + eps32) if variant == 'eps_outside' else 1.0 / (var + eps32).sqrt()
    assert mean.dtype == torch.float32 and rstd.dtype == torch.float32
    return mean, rstd


def ln_fwd_mirror(x, gamma, beta, prec, eps=EPS, variant=None):
    """the stored output of an fp32 LayerNorm, read back in fp64"""
    mean, rstd = _ln_stats32(x, eps, variant)
    return stored64((x - mean) * rstd * gamma + beta, prec)


def ln_bwd_mirror(x, dy, gamma, res, prec, eps=EPS, variant=None):
    """xhat = (x - mean) rstd; g = dy gamma; dx = rstd (g - mean(g) - xhat mean(g xhat)) [+ res]"""
    d = x.shape[-1]
    mean, rstd = _ln_stats32(x, eps, variant)
    xhat, g = (x - mean) * rstd, dy * gamma
    mg, mgx = g.sum(-1, keepdim=True) / d, (g * xhat).sum(-1, keepdim=True) / d
    r = rstd * (g - mg if variant == 'no_xhat_term' else g - mg - xhat * mgx)
    return stored64(r if res is None else r + res, prec)


# ------------------------------------------------------------------ soft-max rows
def scores_for(rows, n_valid, ld, gen, prec, slack=NAN):
    """stored fp32 scores [rows][ld] (bf16 kernels: bf16 values; pair kernels read fp32): 8 randn, and planted at rows 1, 2, 3 all
    valid scores equal; all -300 with +300 in the last valid column; the maximum in column 0.  Columns n_valid .. ld hold `slack`."""
    assert rows >= 4
    s = 8 * torch.randn(rows, ld, generator=gen)
    s[SM_EQUAL] = 2.5
    s[SM_ONE_HOT] = -300
    s[SM_ONE_HOT, n_valid - 1] = 300
    s[SM_MAX_FIRST, 0] = 48
    if prec == 'bf16':
        s = s.to(torch.bfloat16).float()
    s[:, n_valid:] = slack
    return s


def sm_fwd_ref(s, n_valid, scale):
    return torch.softmax(scale * s[:, :n_valid].double(), -1)


def sm_fwd_bound(ref, prec):
    return ULP[prec] * ref + 1e-6


def sm_bwd_ref(p, dp, n_valid, scale):
    """scale * P (dP - sum_k P_k dP_k) on the stored P and dP in fp64, by torch's own soft-max derivative"""
    p64, dp64 = p[:, :n_valid].double().contiguous(), dp[:, :n_valid].double().contiguous()
    return scale * torch.ops.aten._softmax_backward_data(dp64, p64, -1, torch.float64)


def sm_bwd_ref_from_scores(s, dp, n_valid, scale):
    sr = s[:, :n_valid].double().requires_grad_(True)
    gs, = torch.autograd.grad(torch.softmax(scale * sr, -1), sr, grad_outputs=dp[:, :n_valid].double())
    return gs


def sm_bwd_bound(p, dp, n_valid, scale, prec, dot_roundings=None):
    """dot_roundings: another count than DOT_ROUNDINGS[prec], for the CPU tests that show why the term and the count are needed"""
    ref = sm_bwd_ref(p, dp, n_valid, scale)
    p64, dp64 = p[:, :n_valid].double(), dp[:, :n_valid].double()
    two = ULP[prec] * ref.abs() + 1e-6 * ref.abs().amax(-1, keepdim=True)
    dot_term = 2.0 ** -24 * scale * p64.abs() * (p64 * dp64).abs().sum(-1, keepdim=True)
    return two + (DOT_ROUNDINGS[prec] if dot_roundings is None else dot_roundings) * dot_term


_sm_cache = {}


def sm_case(prec, shape, rows, scale, slack=NAN):
    """scores [rows][ld_in]; the backward's P = the stored fp64 soft-max [rows][ld_out] and dP = randn [rows][ld_in] (bf16 values
    for the bf16 kernels, fp32 for the pair kernels), every slack column `slack` (a pair: the scores' slack, that of P and dP).
    Drawn once: not to be written to."""
    key = (prec, shape, rows, scale, str(slack))
    if key not in _sm_cache:
        n_valid, ld_in, ld_out = shape
        g = torch.Generator().manual_seed(200000 + 1000 * n_valid + 10 * rows + ld_out)
        s_slack, slack = slack if isinstance(slack, tuple) else (slack, slack)
        s = scores_for(rows, n_valid, ld_in, g, prec, s_slack)
        p = torch.full((rows, ld_out), slack, dtype=torch.float32)
        p[:, :n_valid] = store(sm_fwd_ref(s, n_valid, scale).float(), prec)
        dp = torch.randn(rows, ld_in, generator=g)
        if prec == 'bf16':
            dp = dp.to(torch.bfloat16).float()
        dp[:, n_valid:] = slack
        _sm_cache[key] = dict(s=s, p=p, dp=dp)
    return _sm_cache[key]


def sm_cases(prec):
    """(shape, rows) of every soft-max case"""
    extra_rows, extra_shape = SM_ROWS_EXTRA[prec]
    return [(shape, 6) for shape in SM_SHAPES[prec]] + [(extra_shape, extra_rows)]


def sm_fwd_mirror(s, n_valid, scale, prec, variant=None):
    """exp(s * scale - max) / sum in fp32 over the valid columns, stored; [rows][n_valid] in fp64"""
    n = n_valid + 1 if variant == 'off_by_one' else n_valid
    t = s[:, :n] * torch.tensor(scale, dtype=torch.float32)
    e = torch.exp(t - t.amax(-1, keepdim=True))
    return stored64(e / e.sum(-1, keepdim=True), prec)[:, :n_valid]


def lane_dot32(a, b, per_lane):
    """sum_k a_k b_k per row as one wave forms it in fp32: lane l takes columns per_lane * l .. (the pair kernels' layout, 4 per
    lane) or, per_lane = 16, its vectors l and l + 64 of eight columns (the bf16 kernels'), accumulates them in order with fused
    multiply-adds, and six butterfly steps add the 64 lanes.  fp32 products are exact in fp64, so float(acc + a * b) is the fma."""
    rows, n = a.shape
    pa, pb = torch.zeros(rows, 64 * per_lane, dtype=torch.float64), torch.zeros(rows, 64 * per_lane, dtype=torch.float64)
    pa[:, :n], pb[:, :n] = a, b
    if per_lane == 16:
        pa, pb = (t.view(rows, 2, 64, 8).permute(0, 2, 1, 3).reshape(rows, 64, 16) for t in (pa, pb))
    else:
        pa, pb = pa.view(rows, 64, per_lane), pb.view(rows, 64, per_lane)
    acc = torch.zeros(rows, 64, dtype=torch.float32)
    for j in range(per_lane):
        acc = (acc.double() + pa[:, :, j] * pb[:, :, j]).float()
    lanes = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ off]
    assert acc.dtype == torch.float32
    return acc[:, :1]


def sm_bwd_mirror(p, dp, n_valid, scale, prec, variant=None, order=None):
    """order='lanes': the dot in the kernel's own order (lane_dot32) instead of torch's sum"""
    n = min(p.shape[1], dp.shape[1]) if variant == 'dot_over_ld' else n_valid
    dot = lane_dot32(p[:, :n], dp[:, :n], 16 if prec == 'bf16' else 4) if order == 'lanes' else (p[:, :n] * dp[:, :n]).sum(-1, keepdim=True)
    sc = torch.tensor(scale, dtype=torch.float32)
    return stored64(sc * p[:, :n_valid] * (dp[:, :n_valid] - dot), prec)


# ------------------------------------------------------------------ GELU
def gelu_patterns():
    """Every bf16 bit pattern with u == 0 (both signs) or 2^-100 <= |u| < 2^127, as int16 bits: 2 + 2 * 227 * 128 = 58,114
    patterns.  Subnormals, the binades below 2^-100 and the top binade are left out: there the order of the fp32 operations decides
    between a finite and a non-finite (or flushed) result, and no engine produces such activations; infinities and NaN likewise."""
    e = torch.arange(127 - 100, 127 + 127, dtype=torch.int32)                 # biased exponents of 2^-100 .. 2^126
    mag = (e.view(-1, 1) * 128 + torch.arange(128, dtype=torch.int32).view(1, -1)).reshape(-1)
    bits = torch.cat([torch.tensor([0, 0x8000], dtype=torch.int32), mag, mag | 0x8000])
    return torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16)


def gelu_operands():
    """the pattern set as a bf16 tensor, padded with +0 to a multiple of 8 -> (operands, number of patterns)"""
    bits = gelu_patterns()
    n = bits.numel()
    pad = torch.zeros((-n) % 8, dtype=torch.int16)
    return torch.cat([bits, pad]).view(torch.bfloat16), n


def gelu_ref(u):
    """-> gelu(u) and gelu'(u) in fp64: torch.nn.functional.gelu and its autograd"""
    ur = u.double().requires_grad_(True)
    y = F.gelu(ur)
    dydu, = torch.autograd.grad(y.sum(), ur)
    return y.detach(), dydu


def gelu_bound(ref, u):
    return 2.0 ** -7 * ref.abs() + 2.0 ** -23 * u.double().abs()


def gelu_grad_bound(dref, u, dh):
    """dref = gelu'(u) in fp64, dh a number or a tensor"""
    dh = torch.as_tensor(dh, dtype=torch.float64).abs()
    return dh * (2.0 ** -7 * dref.abs() + 2.0 ** -22 * (1 + u.double().abs().clamp(max=10)))


def gelu_mirror(u, variant=None):
    v = u.float()
    if variant == 'tanh':
        r = 0.5 * v * (1 + torch.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v * v * v)))
    else:
        r = 0.5 * v * (1 + torch.erf(v * 0.70710678118654752))
    return r.to(torch.bfloat16).double()


def gelu_grad_mirror(u, dh, variant=None):
    v = u.float()
    r = 0.5 * (1 + torch.erf(v * 0.70710678118654752))
    if variant != 'no_v_phi':
        r = r + v * 0.3989422804014327 * torch.exp(-0.5 * v * v)
    return (torch.as_tensor(dh, dtype=torch.float32) * r).to(torch.bfloat16).double()
