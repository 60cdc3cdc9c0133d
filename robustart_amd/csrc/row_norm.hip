// Row LayerNorm over the last dim, forward and backward to the input, for gfx950: one kernel per direction, instantiated for bf16
// storage and for hi + lo pair storage (value = hi + lo, the reference-precision engines' format).  The plain row kernels every engine
// calls through model/engine_base.py (_ln, _ln_bwd); the skeleton and what the two storages do differently are in rart_row_norm.h.
// The backward that also reduces dgamma / dbeta, k_layernorm_bwd_full, is in csrc/vit_bwd.hip.
#include "rart_row_norm.h"

namespace {
using namespace rart_bf16;
constexpr int kBlock = 256;

// y = (x - mean) rstd gamma + beta.  (Round 5, scratch/r5/time_layernorm.py: 36.4 us per launch on bf16 [256 x 197][768] = 4.25 TB/s on
// input + output; a wave walking eight rows with gamma / beta in registers and the next row prefetched was SLOWER, 49.2 us: one row per wave
// keeps far more rows in flight, and the 6 KB of gamma / beta per row are L1 hits.)
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_layernorm(const uint16_t* __restrict__ xh, const uint16_t* __restrict__ xl,
                                                      const float* __restrict__ g, const float* __restrict__ b,
                                                      uint16_t* __restrict__ oh, uint16_t* __restrict__ ol, int rows, int d,
                                                      long long in_stride, long long out_stride, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = d / 8;
  float xr[2][8], mean, rstd;
  row_load<PAIR>(xh + (size_t)row * in_stride, xl + (size_t)row * in_stride, nv, lane, xr);
  ln_row_stats<PAIR>(xr, nv, lane, d, eps, mean, rstd);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int vi = lane + 64 * k;
    if (vi < nv) {
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = (xr[k][j] - mean) * rstd * g[vi * 8 + j] + b[vi * 8 + j];
      row_store8<PAIR>(oh + (size_t)row * out_stride, ol + (size_t)row * out_stride, (size_t)vi * 8, r);
    }
  }
}

// xhat = (x - mean) rstd; g = dy gamma; dx = rstd (g - mean(g) - xhat mean(g xhat)) [+ res]; statistics recomputed from x.  The pair
// instance reads x and dy for the last time: non-temporal (65.63 -> 65.34 ms per reference-precision ViT-B/16 gradient evaluation)
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_layernorm_bwd(const uint16_t* __restrict__ dyh, const uint16_t* __restrict__ dyl,
                                                          const uint16_t* __restrict__ xh, const uint16_t* __restrict__ xl,
                                                          const float* __restrict__ gamma, const uint16_t* __restrict__ rh,
                                                          const uint16_t* __restrict__ rl, uint16_t* __restrict__ oh,
                                                          uint16_t* __restrict__ ol, int rows, int d, long long dy_stride,
                                                          long long x_stride, long long res_stride, long long dx_stride, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = d / 8;
  float xr[2][8], gr[2][8], mean, rstd;
  row_load<PAIR, PAIR>(xh + (size_t)row * x_stride, xl + (size_t)row * x_stride, nv, lane, xr);
  row_load<PAIR, PAIR>(dyh + (size_t)row * dy_stride, dyl + (size_t)row * dy_stride, nv, lane, gr);
  ln_row_stats<PAIR>(xr, nv, lane, d, eps, mean, rstd);
  float sg = 0.f, sgx = 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int vi = lane + 64 * k;
    if (vi < nv) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        gr[k][j] *= gamma[vi * 8 + j];
        xr[k][j] = (xr[k][j] - mean) * rstd;                     // xhat
        sg += gr[k][j];
        sgx += gr[k][j] * xr[k][j];
      }
    }
  }
  const float mg = rart_wave_sum(sg) / (float)d, mgx = rart_wave_sum(sgx) / (float)d;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int vi = lane + 64 * k;
    if (vi < nv) {
      float rs[8];
      if (rh) row_load8<PAIR>(rh + (size_t)row * res_stride, rl + (size_t)row * res_stride, (size_t)vi * 8, rs);
      ln_store_dx8<PAIR>(gr[k], xr[k], rstd, mg, mgx, rh != nullptr, rs, oh + (size_t)row * dx_stride, ol + (size_t)row * dx_stride,
                         (size_t)vi * 8);
    }
  }
}

// `what` is the entry's name: PAIR = false ignores the lo pointers (the bf16 entries pass null)
template <bool PAIR>
int launch_layernorm(const void* xh, const void* xl, const float* gamma, const float* beta, void* oh, void* ol, int rows, int dim,
                     int64_t in_row_stride, int64_t out_row_stride, float eps, rart_stream_t stream, const char* what) {
  RART_CHECK_ARG(xh && gamma && beta && oh && (!PAIR || (xl && ol)) && rows > 0 && dim > 0, "%s: bad arguments", what);
  RART_CHECK_ARG(dim % 8 == 0 && dim <= 1024 && in_row_stride % 8 == 0 && out_row_stride % 8 == 0,
                 "%s: dim a multiple of 8, at most 1024; strides multiples of 8", what);
  hipLaunchKernelGGL(k_layernorm<PAIR>, dim3((rows + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const uint16_t*)xh, (const uint16_t*)xl, gamma, beta, (uint16_t*)oh, (uint16_t*)ol, rows, dim,
                     (long long)in_row_stride, (long long)out_row_stride, eps);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}

template <bool PAIR>
int launch_layernorm_bwd(const void* dyh, const void* dyl, const void* xh, const void* xl, const float* gamma, const void* rh,
                         const void* rl, void* oh, void* ol, int rows, int dim, int64_t dy_row_stride, int64_t x_row_stride,
                         int64_t res_row_stride, int64_t dx_row_stride, float eps, rart_stream_t stream, const char* what) {
  RART_CHECK_ARG(dyh && xh && gamma && oh && (!PAIR || (dyl && xl && ol && ((rh == nullptr) == (rl == nullptr)))) && rows > 0 && dim > 0,
                 "%s: bad arguments", what);
  RART_CHECK_ARG(dim % 8 == 0 && dim <= 1024 && dy_row_stride % 8 == 0 && x_row_stride % 8 == 0 && res_row_stride % 8 == 0 &&
                     dx_row_stride % 8 == 0, "%s: dim a multiple of 8, at most 1024; strides multiples of 8", what);
  hipLaunchKernelGGL(k_layernorm_bwd<PAIR>, dim3((rows + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const uint16_t*)dyh, (const uint16_t*)dyl, (const uint16_t*)xh, (const uint16_t*)xl, gamma, (const uint16_t*)rh,
                     (const uint16_t*)rl, (uint16_t*)oh, (uint16_t*)ol, rows, dim, (long long)dy_row_stride, (long long)x_row_stride,
                     (long long)res_row_stride, (long long)dx_row_stride, eps);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}
}  // namespace

extern "C" {

int rart_layernorm_bf16(const void* x, const float* gamma, const float* beta, void* out, int rows, int dim,
                        int64_t in_row_stride, int64_t out_row_stride, float eps, rart_stream_t stream) {
  return launch_layernorm<false>(x, nullptr, gamma, beta, out, nullptr, rows, dim, in_row_stride, out_row_stride, eps, stream,
                                 "rart_layernorm_bf16");
}

int rart_layernorm_pair(const void* x_hi, const void* x_lo, const float* gamma, const float* beta, void* out_hi, void* out_lo, int rows,
                        int dim, int64_t in_row_stride, int64_t out_row_stride, float eps, rart_stream_t stream) {
  return launch_layernorm<true>(x_hi, x_lo, gamma, beta, out_hi, out_lo, rows, dim, in_row_stride, out_row_stride, eps, stream,
                                "rart_layernorm_pair");
}

int rart_layernorm_bwd_bf16(const void* dy, const void* x, const float* gamma, const void* res, void* dx, int rows, int dim,
                            int64_t dy_row_stride, int64_t x_row_stride, int64_t res_row_stride, int64_t dx_row_stride,
                            float eps, rart_stream_t stream) {
  return launch_layernorm_bwd<false>(dy, nullptr, x, nullptr, gamma, res, nullptr, dx, nullptr, rows, dim, dy_row_stride, x_row_stride,
                                     res_row_stride, dx_row_stride, eps, stream, "rart_layernorm_bwd_bf16");
}

int rart_layernorm_bwd_pair(const void* dy_hi, const void* dy_lo, const void* x_hi, const void* x_lo, const float* gamma,
                            const void* res_hi, const void* res_lo, void* dx_hi, void* dx_lo, int rows, int dim, int64_t dy_row_stride,
                            int64_t x_row_stride, int64_t res_row_stride, int64_t dx_row_stride, float eps, rart_stream_t stream) {
  return launch_layernorm_bwd<true>(dy_hi, dy_lo, x_hi, x_lo, gamma, res_hi, res_lo, dx_hi, dx_lo, rows, dim, dy_row_stride,
                                    x_row_stride, res_row_stride, dx_row_stride, eps, stream, "rart_layernorm_bwd_pair");
}

}  // extern "C"
