// Global Response Norm (GRN) of the ConvNeXt-V2-B engine (model `convnextv2_base`, robustart_amd/model/convnext_engine.py) for gfx950:
// its statistics, its application and its backward to the input, fused with GELU' of the fc1 pre-activation.  Every kernel exists in
// two precisions: bf16 storage (the fast engine) and PAIRS of bf16 planes, value = hi + lo (the reference-precision "fp32x" engine).
// Arithmetic and statistics are fp32.  Activations are NHWC, per image [p][c] with P = H * W pixels and C = the 4x hidden width.
//
//   forward    G[n][c] = sqrt(sum_p y^2),  m = mean_c G,  z = y * (1 + w[c] G[c] / (m + eps)) + b[c]
//   backward   a[n][c] = w[c] * sum_p g y,  s = sum_c a G,  beta[c] = a[c] / (m + eps) - s / (C (m + eps)^2),
//              dh = (g (1 + w[c] G[c] / (m + eps)) + y beta[c] / G[c]) * gelu'(u)     (the y term is 0 where G[c] == 0)
//
// Reductions over pixels (stats, bwd_reduce): one workgroup per (image, 128-channel slice) walks all P pixels.  Lane (l % 16) owns
// eight consecutive channels (one 16-byte load per plane), row (l / 16) every 16th pixel; the 16 row sums meet in LDS and are added
// in a fixed order.  The split depends on C alone -- never on the batch -- and there are no atomics, so an image's statistics are
// bit-identical whatever batch it is in and on every call.  At ConvNeXt-V2-B's four stages (P = 3136 .. 49, C = 512 .. 4096) a
// batch of 256 gives 1024 .. 8192 workgroups.
// Per-pixel kernels (apply, bwd_apply): one workgroup per (image, tile of about 32768 / C pixels).  Each workgroup first forms the
// per-image scalars (m, and s for the backward) with a fixed-order block sum over the C statistics of its image, then the per-channel
// factors into LDS (2 x C fp32), then streams its tile eight channels per lane.  The output may alias the input it replaces
// (z over y, dh over g): every element is read and written by the same lane.
// Training (bf16 only; robustart_amd/model/convnext_train_engine.py): rart_cnx_grn_bwd_reduce_train_bf16 adds GRN's parameter gradients,
//   dw[c] = sum_n N[n][c] sum_p g y,  db[c] = sum_n sum_p g,  N = G / (m + eps),
// to the bwd_reduce pass: the same workgroup walk also sums g, forms 1 / (m + eps) with k_grn_apply's block sum and writes per-image
// partials to a workspace ([n][2][c] fp32), and k_grn_param_fold adds them over the images in a fixed order.  `a` keeps the bits of
// rart_cnx_grn_bwd_reduce_bf16 (same FMAs, same order), so rart_cnx_grn_bwd_apply_bf16 consumes it unchanged.
// Reference: timm's GlobalResponseNorm (channels-last) inside GlobalResponseNormMlp, restated in robustart_amd/model/convnext_torch.py.
#include "rart_bf16_helpers.h"
#include "rart_gemm_pair_dev.h"   // gp_gelu_grad

namespace {
using namespace rart_bf16;
constexpr int kBlock = 256;
constexpr int kSliceLanes = 16;                         // lanes across channels in the reductions: 16 x 8 = 128 channels
constexpr int kSlice = kSliceLanes * 8;
constexpr int kRows = kBlock / kSliceLanes;             // pixel rows per pass
constexpr int kMaxC = 4096;                             // per-channel factors in LDS: 2 x C x 4 bytes <= 32 KB
constexpr int kTileElems = 32768;                       // elements per workgroup of the per-pixel kernels

// sum of one value per thread over the workgroup, the same fixed order in every workgroup; s_red: kBlock / 64 floats
__device__ __forceinline__ float block_sum(float v, float* s_red) {
  v = rart_wave_sum(v);
  __syncthreads();                                      // s_red may still be read by a previous call
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < kBlock / 64; ++k) t += s_red[k];
  return t;
}

// grid (slices, n): out[n][c] = sqrt(sum_p y^2) (GRAD = false) or w[c] * sum_p g y (GRAD = true).
// TRAIN (with GRAD): the same g y sums, the same FMAs in the same order and the same row fold, so `out` keeps its bits; in the same
// pass sum_p g, and the GRN parameter-gradient partials of image n go to part[n][0][c] = N[n][c] * sum_p g y, part[n][1][c] = sum_p g.
template <bool PAIR, bool GRAD, bool TRAIN = false>
__global__ __launch_bounds__(kBlock) void k_grn_reduce(const uint16_t* __restrict__ yh, const uint16_t* __restrict__ yl,
                                                       const uint16_t* __restrict__ gh, const uint16_t* __restrict__ gl,
                                                       const float* __restrict__ w, float* __restrict__ out, int P, int C,
                                                       const float* __restrict__ G, float eps, float* __restrict__ part) {
  __shared__ float s_part[kRows][kSlice];
  __shared__ float s_partg[TRAIN ? kRows : 1][kSlice];
  __shared__ float s_red[kBlock / 64];
  const int lc = threadIdx.x % kSliceLanes, row = threadIdx.x / kSliceLanes;
  const int c = blockIdx.x * kSlice + lc * 8;
  const size_t img = (size_t)blockIdx.y * P * C;
  float acc[8], accg[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = accg[k] = 0.f;
  if (c < C) {
    int p = row;
    for (; p + 3 * kRows < P; p += 4 * kRows) {        // four independent loads in flight, summed in pixel order
      float y[4][8], g[4][8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const size_t o = img + (size_t)(p + q * kRows) * C + c;
        ld8<PAIR>(yh, yl, o, y[q]);
        if (GRAD) ld8<PAIR>(gh, gl, o, g[q]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = fmaf(GRAD ? g[q][k] : y[q][k], y[q][k], acc[k]);
      if (TRAIN) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int k = 0; k < 8; ++k) accg[k] += g[q][k];
      }
    }
    for (; p < P; p += kRows) {
      float y[8], g[8];
      const size_t o = img + (size_t)p * C + c;
      ld8<PAIR>(yh, yl, o, y);
      if (GRAD) ld8<PAIR>(gh, gl, o, g);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = fmaf(GRAD ? g[k] : y[k], y[k], acc[k]);
      if (TRAIN) {
#pragma unroll
        for (int k = 0; k < 8; ++k) accg[k] += g[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) s_part[row][lc * 8 + k] = acc[k];
  if (TRAIN) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s_partg[row][lc * 8 + k] = accg[k];
  }
  float inv = 0.f;
  if (TRAIN) {                                          // 1 / (m + eps), formed exactly as k_grn_apply forms it
    const float* Gn = G + (size_t)blockIdx.y * C;
    float t = 0.f;
    for (int cc = threadIdx.x; cc < C; cc += kBlock) t += Gn[cc];
    inv = 1.0f / (block_sum(t, s_red) / (float)C + eps);
  }
  __syncthreads();
  if (threadIdx.x < kSlice) {
    const int cc = blockIdx.x * kSlice + threadIdx.x;
    if (cc < C) {
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < kRows; ++r) t += s_part[r][threadIdx.x];
      out[(size_t)blockIdx.y * C + cc] = GRAD ? w[cc] * t : sqrtf(t);
      if (TRAIN) {
        float tg = 0.f;
#pragma unroll
        for (int r = 0; r < kRows; ++r) tg += s_partg[r][threadIdx.x];
        float* pn = part + (size_t)blockIdx.y * 2 * C;
        const float nc = G[(size_t)blockIdx.y * C + cc] * inv;
        pn[cc] = nc * t;
        pn[C + cc] = tg;
      }
    }
  }
}

// grid (ceil(C / 32), 2): dw[c] (blockIdx.y 0) or db[c] (1) (+)= sum over images of part[n][blockIdx.y][c].  8 threads per channel
// each add a contiguous eighth of the images, then one thread adds the eight sums in segment order.
constexpr int kFoldLanes = 32;
constexpr int kFoldSeg = kBlock / kFoldLanes;
__global__ __launch_bounds__(kBlock) void k_grn_param_fold(const float* __restrict__ part, int N, int C, float* __restrict__ dw,
                                                           float* __restrict__ db, int accumulate) {
  __shared__ float s_seg[kBlock];
  const int cl = threadIdx.x % kFoldLanes, seg = threadIdx.x / kFoldLanes, c = blockIdx.x * kFoldLanes + cl, j = blockIdx.y;
  const int per = (N + kFoldSeg - 1) / kFoldSeg, q0 = seg * per, q1 = min(N, q0 + per);
  float s = 0.f;
  if (c < C)
    for (int q = q0; q < q1; ++q) s += part[((size_t)q * 2 + j) * C + c];
  s_seg[threadIdx.x] = s;
  __syncthreads();
  if (seg == 0 && c < C) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < kFoldSeg; ++k) t += s_seg[k * kFoldLanes + cl];
    float* o = (j ? db : dw) + c;
    *o = accumulate ? *o + t : t;
  }
}

// grid (tiles, n): z = y * (1 + w N) + b over pixels [tile * tile_px, + tile_px) of image n.  z may alias y.
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_grn_apply(const uint16_t* yh, const uint16_t* yl, const float* __restrict__ G,
                                                      const float* __restrict__ w, const float* __restrict__ b, uint16_t* zh, uint16_t* zl,
                                                      int P, int C, int tile_px, float eps) {
  extern __shared__ float s_f[];                        // [C] scale 1 + w N, [C] bias
  __shared__ float s_red[kBlock / 64];
  float* s_scale = s_f;
  float* s_bias = s_f + C;
  const float* Gn = G + (size_t)blockIdx.y * C;
  float t = 0.f;
  for (int c = threadIdx.x; c < C; c += kBlock) t += Gn[c];
  const float inv = 1.0f / (block_sum(t, s_red) / (float)C + eps);
  for (int c = threadIdx.x; c < C; c += kBlock) {
    s_scale[c] = fmaf(w[c], Gn[c] * inv, 1.0f);
    s_bias[c] = b[c];
  }
  __syncthreads();
  const int c8 = C / 8;
  const int p0 = blockIdx.x * tile_px, np = min(tile_px, P - p0);
  const size_t base = ((size_t)blockIdx.y * P + p0) * C;
  for (int i = threadIdx.x; i < np * c8; i += kBlock) {
    const int c = (i % c8) * 8;
    const size_t o = base + (size_t)i * 8;
    float v[8];
    ld8<PAIR>(yh, yl, o, v);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = fmaf(v[k], s_scale[c + k], s_bias[c + k]);
    st8<PAIR>(zh, zl, o, v);
  }
}

// grid (tiles, n): dh = (g (1 + w N) + y beta / G) * gelu'(u).  dh may alias g.
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_grn_bwd_apply(const uint16_t* gh, const uint16_t* gl, const uint16_t* __restrict__ yh,
                                                          const uint16_t* __restrict__ yl, const uint16_t* __restrict__ uh,
                                                          const uint16_t* __restrict__ ul, const float* __restrict__ G,
                                                          const float* __restrict__ a, const float* __restrict__ w, uint16_t* dhh,
                                                          uint16_t* dhl, int P, int C, int tile_px, float eps) {
  extern __shared__ float s_f[];                        // [C] 1 + w N, [C] beta / G
  __shared__ float s_red[kBlock / 64];
  float* s_k1 = s_f;
  float* s_k2 = s_f + C;
  const float* Gn = G + (size_t)blockIdx.y * C;
  const float* an = a + (size_t)blockIdx.y * C;
  float tg = 0.f, ts = 0.f;
  for (int c = threadIdx.x; c < C; c += kBlock) {
    tg += Gn[c];
    ts = fmaf(an[c], Gn[c], ts);
  }
  const float me = block_sum(tg, s_red) / (float)C + eps;
  const float s = block_sum(ts, s_red);
  const float inv = 1.0f / me, corr = s / ((float)C * me * me);
  for (int c = threadIdx.x; c < C; c += kBlock) {
    const float gc = Gn[c];
    s_k1[c] = fmaf(w[c], gc * inv, 1.0f);
    s_k2[c] = gc > 0.f ? fmaf(an[c], inv, -corr) / gc : 0.f;
  }
  __syncthreads();
  const int c8 = C / 8;
  const int p0 = blockIdx.x * tile_px, np = min(tile_px, P - p0);
  const size_t base = ((size_t)blockIdx.y * P + p0) * C;
  for (int i = threadIdx.x; i < np * c8; i += kBlock) {
    const int c = (i % c8) * 8;
    const size_t o = base + (size_t)i * 8;
    float g[8], y[8], u[8];
    ld8<PAIR>(gh, gl, o, g);
    ld8<PAIR>(yh, yl, o, y);
    ld8<PAIR>(uh, ul, o, u);
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = fmaf(g[k], s_k1[c + k], y[k] * s_k2[c + k]) * gp_gelu_grad(u[k]);
    st8<PAIR>(dhh, dhl, o, g);
  }
}

bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

bool grn_shape_ok(int n, int p, int c) {
  return n > 0 && n <= 65535 && p > 0 && c > 0 && c % 8 == 0 && c <= kMaxC && (long long)n * p * c < (1ll << 40);
}

int tile_px(int c) { return kTileElems / c > 1 ? kTileElems / c : 1; }

#define GRN_SHAPE_MSG "c a multiple of 8, at most 4096; 0 < n <= 65535, p > 0"

template <bool PAIR, bool GRAD>
int launch_reduce(const void* yh, const void* yl, const void* gh, const void* gl, const float* w, float* out, int n, int p, int c,
                  rart_stream_t stream, const char* what) {
  hipLaunchKernelGGL((k_grn_reduce<PAIR, GRAD>), dim3((c + kSlice - 1) / kSlice, n), dim3(kBlock), 0, (hipStream_t)stream,
                     (const uint16_t*)yh, (const uint16_t*)yl, (const uint16_t*)gh, (const uint16_t*)gl, w, out, p, c, nullptr, 0.f,
                     nullptr);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}

template <bool PAIR>
int launch_apply(const void* yh, const void* yl, const float* G, const float* w, const float* b, void* zh, void* zl, int n, int p, int c,
                 float eps, rart_stream_t stream, const char* what) {
  const int tp = tile_px(c);
  hipLaunchKernelGGL(k_grn_apply<PAIR>, dim3((p + tp - 1) / tp, n), dim3(kBlock), 2 * c * sizeof(float), (hipStream_t)stream,
                     (const uint16_t*)yh, (const uint16_t*)yl, G, w, b, (uint16_t*)zh, (uint16_t*)zl, p, c, tp, eps);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}

template <bool PAIR>
int launch_bwd_apply(const void* gh, const void* gl, const void* yh, const void* yl, const void* uh, const void* ul, const float* G,
                     const float* a, const float* w, void* dhh, void* dhl, int n, int p, int c, float eps, rart_stream_t stream,
                     const char* what) {
  const int tp = tile_px(c);
  hipLaunchKernelGGL(k_grn_bwd_apply<PAIR>, dim3((p + tp - 1) / tp, n), dim3(kBlock), 2 * c * sizeof(float), (hipStream_t)stream,
                     (const uint16_t*)gh, (const uint16_t*)gl, (const uint16_t*)yh, (const uint16_t*)yl, (const uint16_t*)uh,
                     (const uint16_t*)ul, G, a, w, (uint16_t*)dhh, (uint16_t*)dhl, p, c, tp, eps);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}
}  // namespace

int rart_cnx_grn_stats_bf16(const void* y, float* G, int n, int p, int c, rart_stream_t stream) {
  RART_CHECK_ARG(y && G, "rart_cnx_grn_stats_bf16: bad arguments");
  RART_CHECK_ARG(al16(y), "rart_cnx_grn_stats_bf16: y 16-byte aligned");
  RART_CHECK_ARG(grn_shape_ok(n, p, c), "rart_cnx_grn_stats_bf16: " GRN_SHAPE_MSG);
  return launch_reduce<false, false>(y, y, nullptr, nullptr, nullptr, G, n, p, c, stream, "rart_cnx_grn_stats_bf16");
}

int rart_cnx_grn_stats_pair(const void* y_hi, const void* y_lo, float* G, int n, int p, int c, rart_stream_t stream) {
  RART_CHECK_ARG(y_hi && y_lo && G, "rart_cnx_grn_stats_pair: bad arguments");
  RART_CHECK_ARG(al16(y_hi) && al16(y_lo), "rart_cnx_grn_stats_pair: y planes 16-byte aligned");
  RART_CHECK_ARG(grn_shape_ok(n, p, c), "rart_cnx_grn_stats_pair: " GRN_SHAPE_MSG);
  return launch_reduce<true, false>(y_hi, y_lo, nullptr, nullptr, nullptr, G, n, p, c, stream, "rart_cnx_grn_stats_pair");
}

int rart_cnx_grn_apply_bf16(const void* y, const float* G, const float* w, const float* b, void* z, int n, int p, int c, float eps,
                            rart_stream_t stream) {
  RART_CHECK_ARG(y && G && w && b && z, "rart_cnx_grn_apply_bf16: bad arguments");
  RART_CHECK_ARG(al16(y) && al16(z), "rart_cnx_grn_apply_bf16: y / z 16-byte aligned");
  RART_CHECK_ARG(grn_shape_ok(n, p, c), "rart_cnx_grn_apply_bf16: " GRN_SHAPE_MSG);
  return launch_apply<false>(y, y, G, w, b, z, z, n, p, c, eps, stream, "rart_cnx_grn_apply_bf16");
}

int rart_cnx_grn_apply_pair(const void* y_hi, const void* y_lo, const float* G, const float* w, const float* b, void* z_hi, void* z_lo, int n,
                            int p, int c, float eps, rart_stream_t stream) {
  RART_CHECK_ARG(y_hi && y_lo && G && w && b && z_hi && z_lo && (z_hi == y_hi) == (z_lo == y_lo),
                 "rart_cnx_grn_apply_pair: bad arguments (z aliases both planes of y or neither)");
  RART_CHECK_ARG(al16(y_hi) && al16(y_lo) && al16(z_hi) && al16(z_lo), "rart_cnx_grn_apply_pair: y / z planes 16-byte aligned");
  RART_CHECK_ARG(grn_shape_ok(n, p, c), "rart_cnx_grn_apply_pair: " GRN_SHAPE_MSG);
  return launch_apply<true>(y_hi, y_lo, G, w, b, z_hi, z_lo, n, p, c, eps, stream, "rart_cnx_grn_apply_pair");
}

int rart_cnx_grn_bwd_reduce_bf16(const void* g, const void* y, const float* w, float* a, int n, int p, int c, rart_stream_t stream) {
  RART_CHECK_ARG(g && y && w && a, "rart_cnx_grn_bwd_reduce_bf16: bad arguments");
  RART_CHECK_ARG(al16(g) && al16(y), "rart_cnx_grn_bwd_reduce_bf16: g / y 16-byte aligned");
  RART_CHECK_ARG(grn_shape_ok(n, p, c), "rart_cnx_grn_bwd_reduce_bf16: " GRN_SHAPE_MSG);
  return launch_reduce<false, true>(y, y, g, g, w, a, n, p, c, stream, "rart_cnx_grn_bwd_reduce_bf16");
}

int rart_cnx_grn_bwd_reduce_pair(const void* g_hi, const void* g_lo, const void* y_hi, const void* y_lo, const float* w, float* a, int n, int p,
                                 int c, rart_stream_t stream) {
  RART_CHECK_ARG(g_hi && g_lo && y_hi && y_lo && w && a, "rart_cnx_grn_bwd_reduce_pair: bad arguments");
  RART_CHECK_ARG(al16(g_hi) && al16(g_lo) && al16(y_hi) && al16(y_lo), "rart_cnx_grn_bwd_reduce_pair: g / y planes 16-byte aligned");
  RART_CHECK_ARG(grn_shape_ok(n, p, c), "rart_cnx_grn_bwd_reduce_pair: " GRN_SHAPE_MSG);
  return launch_reduce<true, true>(y_hi, y_lo, g_hi, g_lo, w, a, n, p, c, stream, "rart_cnx_grn_bwd_reduce_pair");
}

int rart_cnx_grn_bwd_apply_bf16(const void* g, const void* y, const void* u, const float* G, const float* a, const float* w, void* dh, int n,
                                int p, int c, float eps, rart_stream_t stream) {
  RART_CHECK_ARG(g && y && u && G && a && w && dh && dh != y && dh != u,
                 "rart_cnx_grn_bwd_apply_bf16: bad arguments (dh may alias g, not y or u)");
  RART_CHECK_ARG(al16(g) && al16(y) && al16(u) && al16(dh), "rart_cnx_grn_bwd_apply_bf16: g / y / u / dh 16-byte aligned");
  RART_CHECK_ARG(grn_shape_ok(n, p, c), "rart_cnx_grn_bwd_apply_bf16: " GRN_SHAPE_MSG);
  return launch_bwd_apply<false>(g, g, y, y, u, u, G, a, w, dh, dh, n, p, c, eps, stream, "rart_cnx_grn_bwd_apply_bf16");
}

int rart_cnx_grn_bwd_apply_pair(const void* g_hi, const void* g_lo, const void* y_hi, const void* y_lo, const void* u_hi, const void* u_lo,
                                const float* G, const float* a, const float* w, void* dh_hi, void* dh_lo, int n, int p, int c, float eps,
                                rart_stream_t stream) {
  RART_CHECK_ARG(g_hi && g_lo && y_hi && y_lo && u_hi && u_lo && G && a && w && dh_hi && dh_lo && (dh_hi == g_hi) == (dh_lo == g_lo) &&
                     dh_hi != y_hi && dh_lo != y_lo && dh_hi != u_hi && dh_lo != u_lo,
                 "rart_cnx_grn_bwd_apply_pair: bad arguments (dh may alias both planes of g, not y or u)");
  RART_CHECK_ARG(al16(g_hi) && al16(g_lo) && al16(y_hi) && al16(y_lo) && al16(u_hi) && al16(u_lo) && al16(dh_hi) && al16(dh_lo),
                 "rart_cnx_grn_bwd_apply_pair: planes 16-byte aligned");
  RART_CHECK_ARG(grn_shape_ok(n, p, c), "rart_cnx_grn_bwd_apply_pair: " GRN_SHAPE_MSG);
  return launch_bwd_apply<true>(g_hi, g_lo, y_hi, y_lo, u_hi, u_lo, G, a, w, dh_hi, dh_lo, n, p, c, eps, stream,
                                "rart_cnx_grn_bwd_apply_pair");
}

size_t rart_cnx_grn_param_grad_workspace_bytes(int n, int c) {
  if (!grn_shape_ok(n, 1, c)) return 0;
  return (size_t)n * 2 * c * sizeof(float);
}

int rart_cnx_grn_bwd_reduce_train_bf16(const void* g, const void* y, const float* G, const float* w, float* a, float* dw, float* db, int n,
                                       int p, int c, float eps, int accumulate, void* workspace, size_t workspace_bytes,
                                       rart_stream_t stream) {
  RART_CHECK_ARG(g && y && G && w && a && dw && db && workspace, "rart_cnx_grn_bwd_reduce_train_bf16: bad arguments");
  RART_CHECK_ARG(al16(g) && al16(y), "rart_cnx_grn_bwd_reduce_train_bf16: g / y 16-byte aligned");
  RART_CHECK_ARG(grn_shape_ok(n, p, c), "rart_cnx_grn_bwd_reduce_train_bf16: " GRN_SHAPE_MSG);
  RART_CHECK_ARG(workspace_bytes >= rart_cnx_grn_param_grad_workspace_bytes(n, c),
                 "rart_cnx_grn_bwd_reduce_train_bf16: workspace smaller than rart_cnx_grn_param_grad_workspace_bytes");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((k_grn_reduce<false, true, true>), dim3((c + kSlice - 1) / kSlice, n), dim3(kBlock), 0, st, (const uint16_t*)y,
                     (const uint16_t*)y, (const uint16_t*)g, (const uint16_t*)g, w, a, p, c, G, eps, (float*)workspace);
  RART_CHECK_LAUNCH("rart_cnx_grn_bwd_reduce_train_bf16");
  hipLaunchKernelGGL(k_grn_param_fold, dim3((c + kFoldLanes - 1) / kFoldLanes, 2), dim3(kBlock), 0, st, (const float*)workspace, n, c, dw,
                     db, accumulate);
  RART_CHECK_LAUNCH("rart_cnx_grn_bwd_reduce_train_bf16 (fold)");
  return RART_OK;
}
