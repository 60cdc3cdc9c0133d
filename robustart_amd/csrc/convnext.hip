// Non-GEMM kernels of the ConvNeXt-B engine (model `convnext_base`, robustart_amd/model/convnext_engine.py) for gfx950: the 7x7
// depthwise convolution fused with the LayerNorm behind it, its backward to the input (transposed depthwise convolution + the
// residual gradient), the 4x4 stem patch extraction and the broadcast backward of the global average pool.  Every kernel exists in
// two precisions: bf16 storage (the fast engine) and PAIRS of bf16 planes, value = hi + lo (the reference-precision "fp32x" engine,
// see rart_gemm_pair_bf16).  Arithmetic is fp32 in both; activations are NHWC [n][h][w][c], the layout the GEMMs use.
//
// Depthwise 7x7 + LayerNorm, one workgroup per (image, output row), all C channels:
//   * The conv reads its input straight from global memory (L1 / L2): a thread owns four consecutive channels and a run of kRun = 4
//     consecutive output pixels and slides a 10-pixel register window along each of the 7 input rows (70 8-byte loads per plane for
//     784 FMAs; the 64 lanes of a wave read 256 consecutive channels).  The first form, one channel and 2-byte loads per thread, issued
//     13 load instructions per output and ran at 5 % of HBM bandwidth.
//   * The fp32 conv outputs of the row go to LDS, [w][c] (w * c * 4 bytes), and one wave per pixel then takes the two-pass LayerNorm
//     statistics over the C channels and writes the normalised row.
//   LDS budget (160 KiB per CU): an input halo tile covering a whole output row is 7 x (w + 6) x c elements -- 111 KB in bf16 and 222 KB
//   as a pair at stage 1 (56 x 56 x 128), too much for more than one workgroup per CU (and beyond the CU for pairs); a channel-split
//   tile cannot finish the LayerNorm.  So the halo is streamed through the cache and only the conv output row stays in LDS: w * c = 7168
//   at every ConvNeXt-B stage (56 x 128, 28 x 256, 14 x 512, 7 x 1024 at 224 x 224), 28 KB, five workgroups per CU by LDS.
// The backward keeps the same geometry without LDS: dx = res + the 7x7 correlation of dz with the flipped taps.  The LayerNorm backward
// in front of it is rart_layernorm_bwd_bf16 / rart_layernorm_bwd_pair (statistics recomputed from the kept conv output), because its
// per-pixel reduction over C would have to be recomputed for the 6 halo rows of every output row inside one launch.
// Reference: timm's ConvNeXt block (conv_dw -> LayerNorm eps 1e-6 -> fc1 -> GELU -> fc2 -> gamma -> residual), restated in
// robustart_amd/model/convnext_torch.py.
#include "rart_common.h"
#include "rart_bf16_helpers.h"

namespace {
using namespace rart_bf16;
constexpr int kBlock = 256;
constexpr int kRun = 4;                         // output pixels per thread item along a row
constexpr int kVec = 4;                         // channels per thread item (8-byte loads per plane)
constexpr int kMaxRowElems = 16384;             // w * c of the LDS row (64 KB fp32)

template <bool PAIR>
__device__ __forceinline__ float ldv(const uint16_t* __restrict__ h, const uint16_t* __restrict__ l, size_t i) {
  const float v = bf2f(h[i]);
  return PAIR ? v + bf2f(l[i]) : v;
}
template <bool PAIR>
__device__ __forceinline__ void stv(uint16_t* __restrict__ h, uint16_t* __restrict__ l, size_t i, float v) {
  const uint16_t hb = f2bf(v);
  h[i] = hb;
  if (PAIR) l[i] = f2bf(v - bf2f(hb));
}

// four consecutive channels of one pixel: one 8-byte load per plane
template <bool PAIR>
__device__ __forceinline__ void ld4(const uint16_t* h, const uint16_t* l, size_t i, float* v) {
  const uint2 a = *reinterpret_cast<const uint2*>(h + i);
  v[0] = __uint_as_float(a.x << 16);
  v[1] = __uint_as_float(a.x & 0xFFFF0000u);
  v[2] = __uint_as_float(a.y << 16);
  v[3] = __uint_as_float(a.y & 0xFFFF0000u);
  if (PAIR) {
    const uint2 b = *reinterpret_cast<const uint2*>(l + i);
    v[0] += __uint_as_float(b.x << 16);
    v[1] += __uint_as_float(b.x & 0xFFFF0000u);
    v[2] += __uint_as_float(b.y << 16);
    v[3] += __uint_as_float(b.y & 0xFFFF0000u);
  }
}
template <bool PAIR>
__device__ __forceinline__ void st4(uint16_t* h, uint16_t* l, size_t i, const float* v) {
  uint16_t hb[4], lb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    hb[k] = f2bf(v[k]);
    lb[k] = f2bf(v[k] - bf2f(hb[k]));
  }
  *reinterpret_cast<uint2*>(h + i) = make_uint2((uint32_t)hb[0] | ((uint32_t)hb[1] << 16), (uint32_t)hb[2] | ((uint32_t)hb[3] << 16));
  if (PAIR)
    *reinterpret_cast<uint2*>(l + i) = make_uint2((uint32_t)lb[0] | ((uint32_t)lb[1] << 16), (uint32_t)lb[2] | ((uint32_t)lb[3] << 16));
}

// acc[j][k] += sum over the 7x7 window of output pixel (h, w0 + j), channel c + k.  FLIP: the transposed convolution (taps mirrored).
// wdw: fp32 [49][c], tap-major (tap = dy * 7 + dx of the module's [c][1][7][7] weight).
template <bool PAIR, bool FLIP>
__device__ __forceinline__ void dw_run(const uint16_t* __restrict__ xh, const uint16_t* __restrict__ xl, const float* __restrict__ wdw,
                                       size_t img_off, int h, int w0, int H, int W, int C, int c, float (*acc)[kVec]) {
#pragma unroll 1
  for (int dy = 0; dy < 7; ++dy) {
    const int ih = h + dy - 3;
    if (ih < 0 || ih >= H) continue;                                    // uniform over the workgroup
    const size_t row = img_off + (size_t)ih * W * C + c;
    float in[kRun + 6][kVec];
#pragma unroll
    for (int j = 0; j < kRun + 6; ++j) {
      const int iw = w0 + j - 3;
      if (iw >= 0 && iw < W) {
        ld4<PAIR>(xh, xl, row + (size_t)iw * C, in[j]);
      } else {
#pragma unroll
        for (int k = 0; k < kVec; ++k) in[j][k] = 0.f;
      }
    }
#pragma unroll
    for (int dx = 0; dx < 7; ++dx) {
      const int t = FLIP ? (6 - dy) * 7 + (6 - dx) : dy * 7 + dx;
      const float4 wv = *reinterpret_cast<const float4*>(wdw + (size_t)t * C + c);
      const float wk[kVec] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
      for (int j = 0; j < kRun; ++j)
#pragma unroll
        for (int k = 0; k < kVec; ++k) acc[j][k] = fmaf(in[j + dx][k], wk[k], acc[j][k]);
    }
  }
}

// grid (h, n): out = LayerNorm_c(dwconv7x7(x) + b_dw) * gamma + beta; y (nullable) receives the conv output (the LayerNorm backward's x)
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_dwconv_ln(const uint16_t* __restrict__ xh, const uint16_t* __restrict__ xl,
                                                      const float* __restrict__ wdw, const float* __restrict__ bdw,
                                                      const float* __restrict__ g, const float* __restrict__ b, uint16_t* __restrict__ oh,
                                                      uint16_t* __restrict__ ol, uint16_t* __restrict__ yh, uint16_t* __restrict__ yl, int H,
                                                      int W, int C, float eps) {
  extern __shared__ float s_row[];                                      // [W][C] fp32 conv outputs of this row
  const int h = blockIdx.x;
  const size_t img_off = (size_t)blockIdx.y * H * W * C;
  const int runs = (W + kRun - 1) / kRun, nq = C / kVec;
  for (int it = threadIdx.x; it < nq * runs; it += kBlock) {
    const int c = (it % nq) * kVec, w0 = (it / nq) * kRun;
    const float4 bv = *reinterpret_cast<const float4*>(bdw + c);
    float acc[kRun][kVec];
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
      acc[j][0] = bv.x;
      acc[j][1] = bv.y;
      acc[j][2] = bv.z;
      acc[j][3] = bv.w;
    }
    dw_run<PAIR, false>(xh, xl, wdw, img_off, h, w0, H, W, C, c, acc);
#pragma unroll
    for (int j = 0; j < kRun; ++j)
      if (w0 + j < W) *reinterpret_cast<float4*>(s_row + (w0 + j) * C + c) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int p = threadIdx.x >> 6; p < W; p += kBlock / 64) {
    const float* r = s_row + p * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += r[c];
    const float mean = rart_wave_sum(s) / (float)C;
    float v = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float t = r[c] - mean;
      v += t * t;
    }
    const float rstd = 1.0f / sqrtf(rart_wave_sum(v) / (float)C + eps);
    const size_t o = img_off + ((size_t)h * W + p) * C;
    for (int c = lane; c < C; c += 64) {
      const float x = r[c];
      stv<PAIR>(oh, ol, o + c, (x - mean) * rstd * g[c] + b[c]);
      if (yh) stv<PAIR>(yh, yl, o + c, x);
    }
  }
}

// grid (h, n): dx = res (nullable) + the transposed 7x7 depthwise convolution of dz.  res may alias dx (read and written by one thread).
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_dwconv_bwd(const uint16_t* __restrict__ dzh, const uint16_t* __restrict__ dzl,
                                                       const float* __restrict__ wdw, const uint16_t* rh, const uint16_t* rl, uint16_t* dxh,
                                                       uint16_t* dxl, int H, int W, int C) {
  const int h = blockIdx.x;
  const size_t img_off = (size_t)blockIdx.y * H * W * C;
  const int runs = (W + kRun - 1) / kRun, nq = C / kVec;
  for (int it = threadIdx.x; it < nq * runs; it += kBlock) {
    const int c = (it % nq) * kVec, w0 = (it / nq) * kRun;
    float acc[kRun][kVec];
#pragma unroll
    for (int j = 0; j < kRun; ++j)
#pragma unroll
      for (int k = 0; k < kVec; ++k) acc[j][k] = 0.f;
    dw_run<PAIR, true>(dzh, dzl, wdw, img_off, h, w0, H, W, C, c, acc);
#pragma unroll
    for (int j = 0; j < kRun; ++j)
      if (w0 + j < W) {
        const size_t o = img_off + ((size_t)h * W + w0 + j) * C + c;
        if (rh) {
          float r[kVec];
          ld4<PAIR>(rh, rl, o, r);
#pragma unroll
          for (int k = 0; k < kVec; ++k) acc[j][k] += r[k];
        }
        st4<PAIR>(dxh, dxl, o, acc[j]);
      }
  }
}

// dz[b][p][c] = dpool[b][c] / hw: the global average pool's backward, eight channels per thread
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_pool_bwd(const uint16_t* __restrict__ dph, const uint16_t* __restrict__ dpl,
                                                     uint16_t* __restrict__ dzh, uint16_t* __restrict__ dzl, int hw, int c, uint32_t total8) {
  const float inv = 1.0f / (float)hw;
  const uint32_t c8 = (uint32_t)c / 8;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < total8; i += gridDim.x * kBlock) {
    const uint32_t cv = i % c8, img = i / (c8 * (uint32_t)hw);
    const size_t src = ((size_t)img * c8 + cv) * 8, dst = (size_t)i * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) stv<PAIR>(dzh, dzl, dst + j, ldv<PAIR>(dph, dpl, src + j) * inv);
  }
}


// out[b][py * gw + px][c * ps * ps + r * ps + s] = (x[b][c][py * ps + r][px * ps + s] - mean) / std as hi and lo bf16 planes, row
// stride ld; columns 3 ps^2 .. ld are zero (K padded to the GEMM's granularity).  Eight columns per thread.
template <bool SRC_U8>
__global__ __launch_bounds__(kBlock) void k_patchify(const void* __restrict__ src, uint16_t* __restrict__ hi, uint16_t* __restrict__ lo,
                                                     int h, int w, int ps, int ld, uint32_t total8, RartNorm3 nm) {
  const uint32_t gw = (uint32_t)(w / ps), gh = (uint32_t)(h / ps), ld8 = (uint32_t)ld / 8, kk = 3u * ps * ps;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < total8; i += gridDim.x * kBlock) {
    const uint32_t k8 = i % ld8, pidx = i / ld8;
    const uint32_t px = pidx % gw, t = pidx / gw, py = t % gh, img = t / gh;
    uint16_t hv[8], lv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t k = k8 * 8 + j;
      float v = 0.f;
      if (k < kk) {
        const uint32_t c = k / (ps * ps), r = (k / ps) % ps, s = k % ps, y = py * ps + r, x = px * ps + s;
        const float v01 = SRC_U8 ? (float)((const uint8_t*)src)[(((size_t)img * h + y) * w + x) * 3 + c] * (1.0f / 255.0f)
                                 : ((const float*)src)[(((size_t)img * 3 + c) * h + y) * w + x];
        v = (v01 - nm.mean[c]) * nm.istd[c];
      }
      hv[j] = f2bf(v);
      lv[j] = f2bf(v - bf2f(hv[j]));
    }
    uint32_t hw4[4], lw4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      hw4[j] = (uint32_t)hv[2 * j] | ((uint32_t)hv[2 * j + 1] << 16);
      lw4[j] = (uint32_t)lv[2 * j] | ((uint32_t)lv[2 * j + 1] << 16);
    }
    reinterpret_cast<uint4*>(hi)[i] = make_uint4(hw4[0], hw4[1], hw4[2], hw4[3]);
    reinterpret_cast<uint4*>(lo)[i] = make_uint4(lw4[0], lw4[1], lw4[2], lw4[3]);
  }
}


// the conv loads four channels per access: 8-byte activation, 16-byte weight / bias alignment
bool al(const void* p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

bool dw_shape_ok(int n, int h, int w, int c) {
  return n > 0 && n <= 65535 && h > 0 && h <= 65535 && w > 0 && c > 0 && c % 8 == 0 && c <= 1024 && (long long)w * c <= kMaxRowElems;
}

template <bool PAIR>
int launch_dwconv_ln(const void* xh, const void* xl, const float* wdw, const float* bdw, const float* g, const float* b, void* oh, void* ol,
                     void* yh, void* yl, int n, int h, int w, int c, float eps, hipStream_t st, const char* what) {
  const size_t lds = (size_t)w * c * sizeof(float);
  if (!rart_raise_dynamic_lds((const void*)k_dwconv_ln<PAIR>, lds, what)) return RART_ERR_HIP;
  hipLaunchKernelGGL(k_dwconv_ln<PAIR>, dim3(h, n), dim3(kBlock), lds, st, (const uint16_t*)xh, (const uint16_t*)xl, wdw, bdw, g, b,
                     (uint16_t*)oh, (uint16_t*)ol, (uint16_t*)yh, (uint16_t*)yl, h, w, c, eps);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}
}  // namespace

int rart_cnx_dwconv_ln_bf16(const void* x, const float* w_dw, const float* b_dw, const float* gamma, const float* beta, void* out,
                            void* y_keep, int n, int h, int w, int c, float eps, rart_stream_t stream) {
  RART_CHECK_ARG(x && w_dw && b_dw && gamma && beta && out && x != out, "rart_cnx_dwconv_ln_bf16: bad arguments");
  RART_CHECK_ARG(al(x, 8) && al(w_dw, 16) && al(b_dw, 16), "rart_cnx_dwconv_ln_bf16: x 8-byte, w_dw / b_dw 16-byte aligned");
  RART_CHECK_ARG(dw_shape_ok(n, h, w, c), "rart_cnx_dwconv_ln_bf16: c a multiple of 8, at most 1024; w * c <= %d; n, h <= 65535",
                 kMaxRowElems);
  return launch_dwconv_ln<false>(x, x, w_dw, b_dw, gamma, beta, out, out, y_keep, y_keep, n, h, w, c, eps, (hipStream_t)stream,
                                 "rart_cnx_dwconv_ln_bf16");
}

int rart_cnx_dwconv_ln_pair(const void* x_hi, const void* x_lo, const float* w_dw, const float* b_dw, const float* gamma, const float* beta,
                            void* out_hi, void* out_lo, void* y_hi, void* y_lo, int n, int h, int w, int c, float eps, rart_stream_t stream) {
  RART_CHECK_ARG(x_hi && x_lo && w_dw && b_dw && gamma && beta && out_hi && out_lo && ((y_hi == nullptr) == (y_lo == nullptr)) &&
                     x_hi != out_hi, "rart_cnx_dwconv_ln_pair: bad arguments");
  RART_CHECK_ARG(al(x_hi, 8) && al(x_lo, 8) && al(w_dw, 16) && al(b_dw, 16), "rart_cnx_dwconv_ln_pair: x 8-byte, w_dw / b_dw 16-byte aligned");
  RART_CHECK_ARG(dw_shape_ok(n, h, w, c), "rart_cnx_dwconv_ln_pair: c a multiple of 8, at most 1024; w * c <= %d; n, h <= 65535",
                 kMaxRowElems);
  return launch_dwconv_ln<true>(x_hi, x_lo, w_dw, b_dw, gamma, beta, out_hi, out_lo, y_hi, y_lo, n, h, w, c, eps, (hipStream_t)stream,
                                "rart_cnx_dwconv_ln_pair");
}

int rart_cnx_dwconv_bwd_bf16(const void* dz, const float* w_dw, const void* res, void* dx, int n, int h, int w, int c, rart_stream_t stream) {
  RART_CHECK_ARG(dz && w_dw && dx && dz != dx, "rart_cnx_dwconv_bwd_bf16: bad arguments (dz must not alias dx)");
  RART_CHECK_ARG(al(dz, 8) && al(res, 8) && al(dx, 8) && al(w_dw, 16), "rart_cnx_dwconv_bwd_bf16: dz / res / dx 8-byte, w_dw 16-byte aligned");
  RART_CHECK_ARG(dw_shape_ok(n, h, w, c), "rart_cnx_dwconv_bwd_bf16: c a multiple of 8, at most 1024; w * c <= %d; n, h <= 65535",
                 kMaxRowElems);
  hipLaunchKernelGGL(k_dwconv_bwd<false>, dim3(h, n), dim3(kBlock), 0, (hipStream_t)stream, (const uint16_t*)dz, (const uint16_t*)dz, w_dw,
                     (const uint16_t*)res, (const uint16_t*)res, (uint16_t*)dx, (uint16_t*)dx, h, w, c);
  RART_CHECK_LAUNCH("rart_cnx_dwconv_bwd_bf16");
  return RART_OK;
}

int rart_cnx_dwconv_bwd_pair(const void* dz_hi, const void* dz_lo, const float* w_dw, const void* res_hi, const void* res_lo, void* dx_hi,
                             void* dx_lo, int n, int h, int w, int c, rart_stream_t stream) {
  RART_CHECK_ARG(dz_hi && dz_lo && w_dw && dx_hi && dx_lo && ((res_hi == nullptr) == (res_lo == nullptr)) && dz_hi != dx_hi && dz_lo != dx_lo,
                 "rart_cnx_dwconv_bwd_pair: bad arguments (dz must not alias dx)");
  RART_CHECK_ARG(al(dz_hi, 8) && al(dz_lo, 8) && al(res_hi, 8) && al(res_lo, 8) && al(dx_hi, 8) && al(dx_lo, 8) && al(w_dw, 16),
                 "rart_cnx_dwconv_bwd_pair: activations 8-byte, w_dw 16-byte aligned");
  RART_CHECK_ARG(dw_shape_ok(n, h, w, c), "rart_cnx_dwconv_bwd_pair: c a multiple of 8, at most 1024; w * c <= %d; n, h <= 65535",
                 kMaxRowElems);
  hipLaunchKernelGGL(k_dwconv_bwd<true>, dim3(h, n), dim3(kBlock), 0, (hipStream_t)stream, (const uint16_t*)dz_hi, (const uint16_t*)dz_lo,
                     w_dw, (const uint16_t*)res_hi, (const uint16_t*)res_lo, (uint16_t*)dx_hi, (uint16_t*)dx_lo, h, w, c);
  RART_CHECK_LAUNCH("rart_cnx_dwconv_bwd_pair");
  return RART_OK;
}

int rart_cnx_pool_bwd_bf16(const void* dpool, void* dz, int n, int hw, int c, rart_stream_t stream) {
  RART_CHECK_ARG(dpool && dz && n > 0 && hw > 0 && c > 0 && c % 8 == 0 && (size_t)n * hw * c / 8 < (1ull << 32),
                 "rart_cnx_pool_bwd_bf16: bad arguments (c a multiple of 8)");
  const size_t total8 = (size_t)n * hw * c / 8;
  hipLaunchKernelGGL(k_pool_bwd<false>, dim3(rart_grid_wide(total8)), dim3(kBlock), 0, (hipStream_t)stream, (const uint16_t*)dpool,
                     (const uint16_t*)dpool, (uint16_t*)dz, (uint16_t*)dz, hw, c, (uint32_t)total8);
  RART_CHECK_LAUNCH("rart_cnx_pool_bwd_bf16");
  return RART_OK;
}

int rart_cnx_pool_bwd_pair(const void* dpool_hi, const void* dpool_lo, void* dz_hi, void* dz_lo, int n, int hw, int c, rart_stream_t stream) {
  RART_CHECK_ARG(dpool_hi && dpool_lo && dz_hi && dz_lo && n > 0 && hw > 0 && c > 0 && c % 8 == 0 && (size_t)n * hw * c / 8 < (1ull << 32),
                 "rart_cnx_pool_bwd_pair: bad arguments (c a multiple of 8)");
  const size_t total8 = (size_t)n * hw * c / 8;
  hipLaunchKernelGGL(k_pool_bwd<true>, dim3(rart_grid_wide(total8)), dim3(kBlock), 0, (hipStream_t)stream, (const uint16_t*)dpool_hi,
                     (const uint16_t*)dpool_lo, (uint16_t*)dz_hi, (uint16_t*)dz_lo, hw, c, (uint32_t)total8);
  RART_CHECK_LAUNCH("rart_cnx_pool_bwd_pair");
  return RART_OK;
}

int rart_cnx_patchify(const void* src, int src_is_u8, void* hi, void* lo, int n, int h, int w, int patch, int ld, const float* mean_host,
                      const float* std_host, rart_stream_t stream) {
  RART_CHECK_ARG(src && hi && lo && n > 0 && patch > 0 && patch <= 8 && h > 0 && w > 0 && h % patch == 0 && w % patch == 0,
                 "rart_cnx_patchify: bad arguments (patch side 1..8 dividing the image)");
  RART_CHECK_ARG(ld >= 3 * patch * patch && ld % 8 == 0 && (size_t)n * (h / patch) * (w / patch) * ld / 8 < (1ull << 32),
                 "rart_cnx_patchify: the row stride ld must be a multiple of 8 and at least 3 * patch^2");
  const RartNorm3 nm = rart_norm3(mean_host, std_host);
  const size_t total8 = (size_t)n * (h / patch) * (w / patch) * ld / 8;
  if (src_is_u8)
    hipLaunchKernelGGL(k_patchify<true>, dim3(rart_grid_wide(total8)), dim3(kBlock), 0, (hipStream_t)stream, src, (uint16_t*)hi, (uint16_t*)lo,
                       h, w, patch, ld, (uint32_t)total8, nm);
  else
    hipLaunchKernelGGL(k_patchify<false>, dim3(rart_grid_wide(total8)), dim3(kBlock), 0, (hipStream_t)stream, src, (uint16_t*)hi, (uint16_t*)lo,
                       h, w, patch, ld, (uint32_t)total8, nm);
  RART_CHECK_LAUNCH("rart_cnx_patchify");
  return RART_OK;
}
