"""The ConvStem chain of `convnext_base_cvst` / `vit_base_cvst` on the HIP kernels: forward and backward-to-image of a list of units
CS(cin, cout) = Conv2d(3x3, stride 2, padding 1) -> LayerNorm over channels -> exact GELU, plus an optional closing 1x1 convolution
(reference module: convstem_torch.ConvStem).  `ConvStem` serves the engine that owns it (ConvNeXtEngine, ViTEngine): it takes that
engine's precision, buffers and GEMM launchers, so there is one code path for 'bf16' and 'bf16x3' / 'fp32x'.

Layout: NHWC activations, rows = (image, y, x).  A unit of c channels keeps its rows ld(c) elements apart, ld(c) = c rounded up to a
power of two (>= 32): the conv mode of rart_gemm_pair_bf16 takes a power-of-two k_per_tap, and 48 / 96 are no multiples of the GEMMs'
32-deep K step.  The columns c .. ld(c) of every activation a convolution reads are ZERO (rart_ln_gelu_* writes them), and so are the
matching weight columns.  Per launch:
  forward   rart_cvst_im2col (image -> hi + lo patch planes [rows][32], 27 valid columns) -> GEMM + bias (unit 1) -> rart_ln_gelu_*
            -> per further unit: the GEMM's conv mode (9 taps, stride 2, k_per_tap = ld(cin)) + bias -> rart_ln_gelu_*
            -> the 1x1 as a plain GEMM into the caller's rows (the token slots of ViT).  The last rart_ln_gelu_* of a chain without a 1x1
            writes the caller's dense [rows][c] matrix (ConvNeXt's stage-0 input).
  backward  (1x1 dgrad GEMM) -> per unit, last to first: rart_ln_gelu_bwd_* against the kept convolution output -> the convolution's
            dgrad as four conv-mode GEMMs, one per input parity (py, px), over the 1, 2, 2 and 4 filter taps that reach that parity,
            each scattering its pixels with destination stride 2 -> ... -> unit 1's dgrad GEMM to fp32 patches -> rart_cvst_col2im_f32.
Kept by the forward: the convolution outputs u_i (the LayerNorm-GELU backward recomputes everything else).  No host synchronisation."""
import ctypes

from .. import _lib
from .engine_base import F_OUT_F32, act, k32, pad_k, rows_mult

IM2COL_LD = 32                   # 3 x 3 x 3 = 27 columns, padded to the K step of both GEMMs
TAPS9 = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]
PARITIES = [(0, 0), (0, 1), (1, 0), (1, 1)]


def row_stride(c):
    """row stride of a c-channel stem activation: c rounded up to a power of two, at least 32"""
    return max(32, 1 << (c - 1).bit_length())


def parity_taps(p):
    """filter indices k of a 3-tap stride-2 padding-1 convolution that reach input parity p, with the output offset of each:
    input 2 g + p = 2 o + k - 1  ->  o = g + (p + 1 - k) / 2"""
    return [(k, (p + 1 - k) // 2) for k in range(3) if (p + 1 - k) % 2 == 0]


class ConvStem:
    def __init__(self, engine, stem):
        self.eng = engine
        self._kept = None            # (B, Himg, Wimg, [u_i]) of the last forward: what `backward` differentiates
        self.refold(stem)

    def refold(self, stem):
        """(Re)build the weight tables from the module `stem` (convstem_torch.ConvStem) in the owning engine's precision"""
        torch = _lib.require_gpu()
        eng = self.eng
        dev, f32, tab = eng.device, eng._f32, eng._table

        self.units = []
        ld_in = None
        for i, (conv, norm) in enumerate(stem.units):
            if conv.kernel_size != (3, 3) or conv.stride != (2, 2) or conv.padding != (1, 1) or conv.groups != 1:
                raise NotImplementedError('ConvStem units are 3x3 stride-2 padding-1 convolutions')
            w = f32(conv.weight)                                                       # [cout][cin][3][3]
            cout, cin = w.shape[0], w.shape[1]
            if cout % 16 or not 32 <= cout <= 1024:
                raise NotImplementedError('ConvStem widths are multiples of 16 in 32 .. 1024 (got %d)' % cout)
            ld = row_stride(cout)
            U = dict(c=cout, ld=ld, bias=f32(conv.bias), g=f32(norm.weight), b=f32(norm.bias), eps=float(norm.eps))
            if i == 0:
                if cin != 3:
                    raise NotImplementedError('the ConvStem reads a 3-channel image')
                w0 = pad_k(w.reshape(cout, 27), IM2COL_LD)                             # [cout][c * 9 + ky * 3 + kx], zero columns 27 .. 31
                U['w'] = eng._input_table(w0, rows_mult(cout))                         # bf16: [hi | hi] taps of the image pair
                U['wd'] = tab(w0, k32(cout), transpose=True)                           # [32][k32(cout)]
            else:
                wp = torch.zeros(cout, 3, 3, ld_in, dtype=torch.float32, device=dev)
                wp[..., :cin] = w.permute(0, 2, 3, 1)
                U['w'] = tab(wp.reshape(cout, 9 * ld_in))                              # k = (ky * 3 + kx) * ld(cin) + c
                U['wd'] = []
                for py, px in PARITIES:                                                # per input parity: [cin][taps * ld(cout)]
                    ks = [(ky, dy, kx, dx) for ky, dy in parity_taps(py) for kx, dx in parity_taps(px)]
                    U['wd'].append(((py, px), [(dy, dx) for _, dy, _, dx in ks],
                                    tab(torch.cat([pad_k(w[:, :, ky, kx].t(), ld) for ky, _, kx, _ in ks], 1))))
            self.units.append(U)
            ld_in = ld
        self.proj = None
        if stem.proj is not None:
            pw = f32(stem.proj.weight)
            if pw.shape[2:] != (1, 1):
                raise NotImplementedError('the closing convolution of a ConvStem is 1x1')
            pw = pw.reshape(pw.shape[0], pw.shape[1])                                  # [D][cin]
            kp = k32(pw.shape[1])
            self.proj = dict(n=pw.shape[0], k=kp, w=tab(pw, kp), wd=tab(pw, transpose=True), bias=f32(stem.proj.bias))

    # ------------------------------------------------------------------ launches
    def _ln_gelu(self, u, U, out, rows, ld_out):
        self.eng._rows('ln_gelu', act(u), U['g'], U['b'], act(out), rows, U['c'], U['ld'], ld_out, U['eps'])

    def _ln_gelu_bwd(self, dy, ld_dy, u, U, dx, rows):
        self.eng._rows('ln_gelu_bwd', act(dy), act(u), U['g'], U['b'], act(dx), rows, U['c'], ld_dy, U['ld'], U['ld'], U['eps'])

    # ------------------------------------------------------------------ forward / backward
    def forward(self, src, src_is_u8, mean, std, B, Himg, Wimg, out, **slot):
        """the stem of the image batch `src` (u8 NHWC or fp32 NCHW in [0,1]) -> `out`: the dense [rows][c_last] matrix of a chain without
        a 1x1, else the 1x1's output rows placed by `slot` (rows_per_image, dst_rows_per_image, dst_row_off of `RowEngine._mm`)"""
        eng = self.eng
        n = len(self.units)
        if Himg % (1 << n) or Wimg % (1 << n):
            raise ValueError('the ConvStem needs image sides that are multiples of %d (got %dx%d)' % (1 << n, Himg, Wimg))
        H, W = Himg // 2, Wimg // 2
        rows = B * H * W
        patches = eng._get('cvst_patches', (2, rows, IM2COL_LD))
        meanf, stdf = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        _lib.check(eng.lib.rart_cvst_im2col(_lib.ptr(src), 1 if src_is_u8 else 0, _lib.ptr(patches[0]), _lib.ptr(patches[1]), B, Himg, Wimg,
                                            IM2COL_LD, meanf, stdf, _lib.stream_ptr()))
        a, kept = None, []
        for i, U in enumerate(self.units):
            c, ld = U['c'], U['ld']
            if i == 0:
                u = eng._act('cvst_u0', (rows, ld))
                eng._input_gemm(patches, U['w'], u, rows, c, IM2COL_LD, ldc=ld, bias=U['bias'])
            else:
                H, W = H // 2, W // 2
                rows = B * H * W
                u = eng._act('cvst_u%d' % i, (rows, ld))
                eng._conv(a, U['w'], u, B, (H, W), (2 * H, 2 * W), self.units[i - 1]['ld'], TAPS9, c, (H, W), ld, (2, 2), (1, 1), (0, 0),
                           bias=U['bias'])
            kept.append(u)
            if i == n - 1 and self.proj is None:
                self._ln_gelu(u, U, out, rows, c)
            else:
                a = eng._act('cvst_a%d' % i, (rows, ld))
                self._ln_gelu(u, U, a, rows, ld)
        if self.proj is not None:
            P = self.proj
            eng._mm(a, P['w'], out, rows, P['n'], P['k'], lda=self.units[-1]['ld'], bias=P['bias'], **slot)
        self._kept = (B, Himg, Wimg, kept)

    def backward(self, g, std, grad=None, **slot):
        """g: the gradient of the last forward's `out` (slot: rows_per_image, src_rows_per_image, src_row_off of its rows)
        -> d(loss)/d(x01) fp32 NCHW (written into `grad` when given)"""
        torch = _lib.require_gpu()
        eng = self.eng
        if self._kept is None:
            raise RuntimeError('ConvStem.backward needs the forward whose output it differentiates')
        B, Himg, Wimg, kept = self._kept
        n = len(self.units)
        H, W = Himg >> n, Wimg >> n
        rows = B * H * W
        last = self.units[-1]
        if self.proj is not None:
            da, ld_da = eng._act('cvst_da%d' % (n - 1), (rows, last['ld'])), last['ld']
            eng._mm(g, self.proj['wd'], da, rows, last['c'], self.proj['n'], ldc=ld_da, **slot)
        else:
            da, ld_da = g, last['c']
        for i in range(n - 1, -1, -1):
            U = self.units[i]
            u = kept[i]                                                  # the forward's convolution output
            assert u.shape[-2:] == (rows, U['ld']), 'kept convolution output %d does not match the geometry' % i
            du = eng._act('cvst_du%d' % i, (rows, U['ld']))
            self._ln_gelu_bwd(da, ld_da, u, U, du, rows)
            if i > 0:
                P = self.units[i - 1]
                da, ld_da = eng._act('cvst_da%d' % (i - 1), (4 * rows, P['ld'])), P['ld']
                for (py, px), taps, w in U['wd']:
                    eng._conv(du, w, da, B, (H, W), (H, W), U['ld'], taps, P['c'], (2 * H, 2 * W), P['ld'], (1, 1), (2, 2), (py, px))
                H, W = 2 * H, 2 * W
                rows = B * H * W
        dpatch = eng._get('cvst_dpatch', (rows, IM2COL_LD), torch.float32)
        U = self.units[0]
        eng._mm(du, U['wd'], dpatch, rows, IM2COL_LD, k32(U['c']), lda=U['ld'], flags=F_OUT_F32)
        if grad is None:
            grad = torch.empty(B, 3, Himg, Wimg, dtype=torch.float32, device=eng.device)
        _lib.check(eng.lib.rart_cvst_col2im_f32(_lib.ptr(dpatch), _lib.ptr(grad), B, Himg, Wimg, IM2COL_LD, (ctypes.c_float * 3)(*std),
                                                _lib.stream_ptr()))
        return grad
