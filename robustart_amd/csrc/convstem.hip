// Non-GEMM kernels of the convolutional stem ("ConvStem") of the robust ConvNeXt-B / ViT-B/16 variants (models `convnext_base_cvst`,
// `vit_base_cvst`; robustart_amd/model/convstem_engine.py) for gfx950.  The stem is a chain of units
//   Conv2d(cin, cout, 3, stride 2, padding 1, bias) -> LayerNorm over the channels of each pixel (eps 1e-6) -> exact GELU;
// the convolutions run on the GEMMs (the first one over the patch matrix written here, the others in conv mode), these kernels are
// what lies between them.  All four are streaming kernels: every element is read once and written once, 16 bytes per access.
//
//   rart_cvst_im2col        image (fp32 NCHW in [0,1] or u8 NHWC) -> the 3x3 / stride-2 / pad-1 patch matrix of the NORMALISED image as
//                           hi (+ lo) bf16 planes [n * h/2 * w/2][ld], column c * 9 + ky * 3 + kx (the weight's own order), zero columns
//                           27 .. ld.  A tap outside the image is 0: the padding is applied to the normalised image, so it is not
//                           (0 - mean) / std.  Eight columns per thread, one 16-byte store per plane.
//   rart_ln_gelu_*          y = GELU(LayerNorm(x) * gamma + beta) per row of a channels-last matrix, rows `ld` elements apart, columns
//                           dim .. ld_out written as zero (the next convolution contracts over the padded width).  Rows are short
//                           (48 .. 384 channels), so a row is served by a GROUP of 8 / 16 / 32 / 64 lanes, eight consecutive channels
//                           per lane (16 bytes per plane; two such chunks per lane only above 512 channels): a wave holds 8 rows
//                           of 48 or 64 channels.  The row stays in registers: mean, then the centred second moment (two passes
//                           over registers, no cancellation at a large mean), then the affine map and GELU.
//   rart_ln_gelu_bwd_*      dx = LayerNorm'(x)^T (dy * GELU'(LayerNorm(x) * gamma + beta)), statistics and the pre-activation recomputed
//                           from the kept convolution output x (nothing saved by the forward, no parameter gradients), same geometry.
//   rart_cvst_col2im_f32    fp32 d(patches) [rows][ld] -> d(loss)/d(x01) [n][3][h][w] including 1 / std.  Gather form: a thread owns
//                           the 2 x 2 pixel block of one patch position and sums, in a fixed order, the one, two or four patch entries that
//                           cover each pixel; no atomics, every pixel written once.
// GELU is the erfc form of the pair GEMM's epilogue (rart_gemm_pair_dev.h: |error| 3.8e-7 in fp32) in both precisions.
#include "rart_bf16_helpers.h"
#include "rart_gemm_pair_dev.h"   // gp_gelu, gp_gelu_grad

namespace {
using namespace rart_bf16;
constexpr int kBlock = 256;

template <bool PAIR>
__device__ __forceinline__ void cs_zero8(uint16_t* __restrict__ h, uint16_t* __restrict__ l, size_t i) {
  *reinterpret_cast<uint4*>(h + i) = make_uint4(0, 0, 0, 0);
  if (PAIR) *reinterpret_cast<uint4*>(l + i) = make_uint4(0, 0, 0, 0);
}
__device__ __forceinline__ void cs_ldf8(const float* __restrict__ p, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
// sum over the LPR lanes (a power of two, aligned) that share a row
template <int LPR>
__device__ __forceinline__ float cs_group_sum(float v) {
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// One row per group of LPR lanes.  BWD = false: out = GELU(LN(x) * g + b).  BWD = true: out = LN'(x)^T (dy * GELU'(LN(x) * g + b)).
// Columns dim .. ld_out of `out` are written as zero.  NCH: 8-channel chunks per lane, 1 for dim <= 8 LPR (every stem width), 2 for the
// 64-lane groups of dim 528 .. 1024.
template <bool PAIR, int LPR, bool BWD, int NCH>
__global__ __launch_bounds__(kBlock) void k_ln_gelu(const uint16_t* __restrict__ xh, const uint16_t* __restrict__ xl,
                                                    const uint16_t* __restrict__ dyh, const uint16_t* __restrict__ dyl,
                                                    const float* __restrict__ g, const float* __restrict__ b, uint16_t* __restrict__ oh,
                                                    uint16_t* __restrict__ ol, int rows, int dim, long long ld_x, long long ld_dy,
                                                    long long ld_out, float eps) {
  constexpr int kRowsPerBlock = kBlock / LPR;
  const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
  const int n8 = dim / 8, pad8 = (int)(ld_out / 8);
  const float inv_dim = 1.0f / (float)dim;
  for (long long r0 = (long long)blockIdx.x * kRowsPerBlock; r0 < rows; r0 += (long long)gridDim.x * kRowsPerBlock) {
    const long long r = r0 + grp;
    const bool live = r < rows;                                          // a dead group still takes part in the shuffles
    float v[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int q = c * LPR + sub;
      if (live && q < n8) {
        ld8<PAIR>(xh, xl, (size_t)(r * ld_x) + (size_t)q * 8, v[c]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[c][j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[c][j];
    }
    const float mean = cs_group_sum<LPR>(s) * inv_dim;
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c * LPR + sub < n8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          v[c][j] -= mean;
          sq = fmaf(v[c][j], v[c][j], sq);
        }
      }
    }
    const float rstd = 1.0f / sqrtf(cs_group_sum<LPR>(sq) * inv_dim + eps);
    if (!BWD) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int q = c * LPR + sub;
        if (live && q < n8) {
          float gv[8], bv[8], y[8];
          cs_ldf8(g + q * 8, gv);
          cs_ldf8(b + q * 8, bv);
#pragma unroll
          for (int j = 0; j < 8; ++j) y[j] = gp_gelu(fmaf(v[c][j] * rstd, gv[j], bv[j]));
          st8<PAIR>(oh, ol, (size_t)(r * ld_out) + (size_t)q * 8, y);
        }
      }
    } else {
      // dxhat = dy * gelu'(z) * gamma;  dx = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat))
      float dh[NCH][8];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int q = c * LPR + sub;
        if (live && q < n8) {
          float gv[8], bv[8], dy[8];
          cs_ldf8(g + q * 8, gv);
          cs_ldf8(b + q * 8, bv);
          ld8<PAIR>(dyh, dyl, (size_t)(r * ld_dy) + (size_t)q * 8, dy);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float xhat = v[c][j] * rstd;
            v[c][j] = xhat;
            dh[c][j] = dy[j] * gp_gelu_grad(fmaf(xhat, gv[j], bv[j])) * gv[j];
            s1 += dh[c][j];
            s2 = fmaf(dh[c][j], xhat, s2);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) dh[c][j] = 0.f;
        }
      }
      const float m1 = cs_group_sum<LPR>(s1) * inv_dim, m2 = cs_group_sum<LPR>(s2) * inv_dim;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int q = c * LPR + sub;
        if (live && q < n8) {
          float y[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) y[j] = rstd * (dh[c][j] - m1 - v[c][j] * m2);
          st8<PAIR>(oh, ol, (size_t)(r * ld_out) + (size_t)q * 8, y);
        }
      }
    }
    if (live)
      for (int q = n8 + sub; q < pad8; q += LPR) cs_zero8<PAIR>(oh, ol, (size_t)(r * ld_out) + (size_t)q * 8);
  }
}

template <bool PAIR, int LPR, bool BWD, int NCH = 1>
void launch_ln_gelu_lpr(const void* xh, const void* xl, const void* dyh, const void* dyl, const float* g, const float* b, void* oh, void* ol,
                        int rows, int dim, long long ld_x, long long ld_dy, long long ld_out, float eps, hipStream_t st) {
  const int rpb = kBlock / LPR;
  const int grid = rart_grid_for(((size_t)rows + rpb - 1) / rpb, 1, 256 * 16);
  hipLaunchKernelGGL((k_ln_gelu<PAIR, LPR, BWD, NCH>), dim3(grid), dim3(kBlock), 0, st, (const uint16_t*)xh, (const uint16_t*)xl,
                     (const uint16_t*)dyh, (const uint16_t*)dyl, g, b, (uint16_t*)oh, (uint16_t*)ol, rows, dim, ld_x, ld_dy, ld_out, eps);
}

bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

template <bool PAIR, bool BWD>
int launch_ln_gelu(const void* xh, const void* xl, const void* dyh, const void* dyl, const float* g, const float* b, void* oh, void* ol,
                   int rows, int dim, long long ld_x, long long ld_dy, long long ld_out, float eps, rart_stream_t stream, const char* what) {
  RART_CHECK_ARG(xh && g && b && oh && (!PAIR || (xl && ol)) && (!BWD || (dyh && (!PAIR || dyl))), "%s: null pointer", what);
  RART_CHECK_ARG(rows > 0 && dim >= 32 && dim <= 1024 && dim % 16 == 0, "%s: dim must be 32 .. 1024 in steps of 16, rows > 0", what);
  RART_CHECK_ARG(ld_x >= dim && ld_x % 8 == 0 && ld_out >= dim && ld_out % 8 == 0 && (!BWD || (ld_dy >= dim && ld_dy % 8 == 0)),
                 "%s: row strides must cover dim and be multiples of 8", what);
  RART_CHECK_ARG(al16(xh) && al16(xl) && al16(dyh) && al16(dyl) && al16(oh) && al16(ol) && al16(g) && al16(b),
                 "%s: every pointer must be 16-byte aligned", what);
  RART_CHECK_ARG(xh != oh, "%s: the output must not alias x", what);
  hipStream_t st = (hipStream_t)stream;
  const int n8 = dim / 8;
  if (n8 <= 8) launch_ln_gelu_lpr<PAIR, 8, BWD>(xh, xl, dyh, dyl, g, b, oh, ol, rows, dim, ld_x, ld_dy, ld_out, eps, st);
  else if (n8 <= 16) launch_ln_gelu_lpr<PAIR, 16, BWD>(xh, xl, dyh, dyl, g, b, oh, ol, rows, dim, ld_x, ld_dy, ld_out, eps, st);
  else if (n8 <= 32) launch_ln_gelu_lpr<PAIR, 32, BWD>(xh, xl, dyh, dyl, g, b, oh, ol, rows, dim, ld_x, ld_dy, ld_out, eps, st);
  else if (n8 <= 64) launch_ln_gelu_lpr<PAIR, 64, BWD>(xh, xl, dyh, dyl, g, b, oh, ol, rows, dim, ld_x, ld_dy, ld_out, eps, st);
  else launch_ln_gelu_lpr<PAIR, 64, BWD, 2>(xh, xl, dyh, dyl, g, b, oh, ol, rows, dim, ld_x, ld_dy, ld_out, eps, st);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}

// hi (and lo, nullable) [n * gh * gw][ld]: column k = c * 9 + ky * 3 + kx holds the normalised pixel (2 oy + ky - 1, 2 ox + kx - 1) of
// channel c, 0 outside the image and for k >= 27.  Eight columns per thread.
template <bool SRC_U8>
__global__ __launch_bounds__(kBlock) void k_cvst_im2col(const void* __restrict__ src, uint16_t* __restrict__ hi, uint16_t* __restrict__ lo,
                                                        int h, int w, int ld, uint32_t total8, RartNorm3 nm) {
  const uint32_t gw = (uint32_t)w / 2, gh = (uint32_t)h / 2, ld8 = (uint32_t)ld / 8;
  // the stride loop counts in 64 bits (total8 may come close to 2^32), an item's index fits 32
  for (uint64_t it = (uint64_t)blockIdx.x * kBlock + threadIdx.x; it < total8; it += (uint64_t)gridDim.x * kBlock) {
    const uint32_t i = (uint32_t)it;
    const uint32_t k8 = i % ld8, pidx = i / ld8;
    const uint32_t ox = pidx % gw, t = pidx / gw, oy = t % gh, img = t / gh;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t k = k8 * 8 + j;
      v[j] = 0.f;
      if (k < 27u) {
        const uint32_t c = k / 9u, ky = (k / 3u) % 3u, kx = k % 3u;
        const int y = (int)(2u * oy + ky) - 1, x = (int)(2u * ox + kx) - 1;
        if (y >= 0 && y < h && x >= 0 && x < w) {
          const float v01 = SRC_U8 ? (float)((const uint8_t*)src)[(((size_t)img * h + y) * w + x) * 3 + c] * (1.0f / 255.0f)
                                   : ((const float*)src)[(((size_t)img * 3 + c) * h + y) * w + x];
          v[j] = (v01 - nm.mean[c]) * nm.istd[c];
        }
      }
    }
    uint4 hv, lv;
    split8(v, hv, lv);
    reinterpret_cast<uint4*>(hi)[i] = hv;
    if (lo) reinterpret_cast<uint4*>(lo)[i] = lv;
  }
}

// One thread per NX horizontally adjacent patch positions (gy, gx): the 2 x 2 pixel block (2 gy + py, 2 gx + px) of each, three channels.
//   (0, 0): tap (1, 1) of (gy, gx)
//   (0, 1): tap (1, 2) of (gy, gx) + tap (1, 0) of (gy, gx + 1)
//   (1, 0): tap (2, 1) of (gy, gx) + tap (0, 1) of (gy + 1, gx)
//   (1, 1): tap (2, 2) of (gy, gx) + (2, 0) of (gy, gx + 1) + (0, 2) of (gy + 1, gx) + (0, 0) of (gy + 1, gx + 1)
// summed in that order; neighbours past the last patch row / column contribute nothing.
template <int NX>
__global__ __launch_bounds__(kBlock) void k_cvst_col2im(const float* __restrict__ dp, float* __restrict__ grad, int h, int w, int ld,
                                                        uint32_t total, RartNorm3 nm) {
  const uint32_t gw = (uint32_t)w / 2, gh = (uint32_t)h / 2, gwn = gw / NX;
  for (uint64_t it = (uint64_t)blockIdx.x * kBlock + threadIdx.x; it < total; it += (uint64_t)gridDim.x * kBlock) {
    const uint32_t i = (uint32_t)it;
    const uint32_t gxn = i % gwn, t = i / gwn, gy = t % gh, img = t / gh;
    const bool down = gy + 1 < gh;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float top[2 * NX], bot[2 * NX];
#pragma unroll
      for (int e = 0; e < NX; ++e) {
        const uint32_t gx = gxn * NX + e;
        const bool right = gx + 1 < gw;
        const float* p00 = dp + ((size_t)(img * gh + gy) * gw + gx) * ld + c * 9;
        const float* p01 = p00 + ld;
        const float* p10 = p00 + (size_t)gw * ld;
        const float* p11 = p10 + ld;
        float a = p00[4];
        float bq = p00[5];
        if (right) bq += p01[3];
        float cq = p00[7];
        if (down) cq += p10[1];
        float dq = p00[8];
        if (right) dq += p01[6];
        if (down) dq += p10[2];
        if (down && right) dq += p11[0];
        top[2 * e] = a * nm.istd[c];
        top[2 * e + 1] = bq * nm.istd[c];
        bot[2 * e] = cq * nm.istd[c];
        bot[2 * e + 1] = dq * nm.istd[c];
      }
      float* o = grad + (((size_t)img * 3 + c) * h + 2 * gy) * w + (size_t)gxn * NX * 2;
      if constexpr (NX == 2) {
        *reinterpret_cast<float4*>(o) = make_float4(top[0], top[1], top[2], top[3]);
        *reinterpret_cast<float4*>(o + w) = make_float4(bot[0], bot[1], bot[2], bot[3]);
      } else {
        *reinterpret_cast<float2*>(o) = make_float2(top[0], top[1]);
        *reinterpret_cast<float2*>(o + w) = make_float2(bot[0], bot[1]);
      }
    }
  }
}
}  // namespace

int rart_cvst_im2col(const void* src, int src_is_u8, void* hi, void* lo, int n, int h, int w, int ld, const float* mean_host,
                     const float* std_host, rart_stream_t stream) {
  RART_CHECK_ARG(src && hi && n > 0 && h > 0 && w > 0, "rart_cvst_im2col: bad arguments");
  if (h % 2 || w % 2) {
    rart_set_error("rart_cvst_im2col: the image sides must be even (got %d x %d)", h, w);
    return RART_ERR_UNSUPPORTED;
  }
  RART_CHECK_ARG(ld >= 32 && ld % 8 == 0 && al16(hi) && al16(lo), "rart_cvst_im2col: ld a multiple of 8 and >= 32, planes 16-byte aligned");
  const size_t total8 = (size_t)n * (h / 2) * (w / 2) * ld / 8;
  RART_CHECK_ARG(total8 < (1ull << 32), "rart_cvst_im2col: too many patches for one launch (split the batch)");
  const RartNorm3 nm = rart_norm3(mean_host, std_host);
  const int grid = rart_grid_wide(total8);
  if (src_is_u8)
    hipLaunchKernelGGL(k_cvst_im2col<true>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, src, (uint16_t*)hi, (uint16_t*)lo, h, w, ld,
                       (uint32_t)total8, nm);
  else
    hipLaunchKernelGGL(k_cvst_im2col<false>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, src, (uint16_t*)hi, (uint16_t*)lo, h, w, ld,
                       (uint32_t)total8, nm);
  RART_CHECK_LAUNCH("rart_cvst_im2col");
  return RART_OK;
}

int rart_cvst_col2im_f32(const float* dpatches, float* grad, int n, int h, int w, int ld, const float* std_host, rart_stream_t stream) {
  RART_CHECK_ARG(dpatches && grad && n > 0 && h > 0 && w > 0 && ld >= 27, "rart_cvst_col2im_f32: bad arguments (ld >= 27)");
  if (h % 2 || w % 2) {
    rart_set_error("rart_cvst_col2im_f32: the image sides must be even (got %d x %d)", h, w);
    return RART_ERR_UNSUPPORTED;
  }
  const size_t positions = (size_t)n * (h / 2) * (w / 2);
  RART_CHECK_ARG(positions < (1ull << 32), "rart_cvst_col2im_f32: too many patches for one launch (split the batch)");
  const RartNorm3 nm = rart_norm3(nullptr, std_host);
  const bool wide = w % 4 == 0 && al16(grad);            // float4 stores: two patch positions per thread
  const size_t total = wide ? positions / 2 : positions;
  const int grid = rart_grid_wide(total);
  if (wide)
    hipLaunchKernelGGL(k_cvst_col2im<2>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, dpatches, grad, h, w, ld, (uint32_t)total, nm);
  else
    hipLaunchKernelGGL(k_cvst_col2im<1>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, dpatches, grad, h, w, ld, (uint32_t)total, nm);
  RART_CHECK_LAUNCH("rart_cvst_col2im_f32");
  return RART_OK;
}

int rart_ln_gelu_bf16(const void* x, const float* gamma, const float* beta, void* out, int rows, int dim, int64_t in_row_stride,
                      int64_t out_row_stride, float eps, rart_stream_t stream) {
  return launch_ln_gelu<false, false>(x, nullptr, nullptr, nullptr, gamma, beta, out, nullptr, rows, dim, in_row_stride, 0, out_row_stride,
                                      eps, stream, "rart_ln_gelu_bf16");
}

int rart_ln_gelu_pair(const void* x_hi, const void* x_lo, const float* gamma, const float* beta, void* out_hi, void* out_lo, int rows,
                      int dim, int64_t in_row_stride, int64_t out_row_stride, float eps, rart_stream_t stream) {
  return launch_ln_gelu<true, false>(x_hi, x_lo, nullptr, nullptr, gamma, beta, out_hi, out_lo, rows, dim, in_row_stride, 0, out_row_stride,
                                     eps, stream, "rart_ln_gelu_pair");
}

int rart_ln_gelu_bwd_bf16(const void* dy, const void* x, const float* gamma, const float* beta, void* dx, int rows, int dim,
                          int64_t dy_row_stride, int64_t x_row_stride, int64_t dx_row_stride, float eps, rart_stream_t stream) {
  return launch_ln_gelu<false, true>(x, nullptr, dy, nullptr, gamma, beta, dx, nullptr, rows, dim, x_row_stride, dy_row_stride,
                                     dx_row_stride, eps, stream, "rart_ln_gelu_bwd_bf16");
}

int rart_ln_gelu_bwd_pair(const void* dy_hi, const void* dy_lo, const void* x_hi, const void* x_lo, const float* gamma, const float* beta,
                          void* dx_hi, void* dx_lo, int rows, int dim, int64_t dy_row_stride, int64_t x_row_stride, int64_t dx_row_stride,
                          float eps, rart_stream_t stream) {
  return launch_ln_gelu<true, true>(x_hi, x_lo, dy_hi, dy_lo, gamma, beta, dx_hi, dx_lo, rows, dim, x_row_stride, dy_row_stride,
                                    dx_row_stride, eps, stream, "rart_ln_gelu_bwd_pair");
}
