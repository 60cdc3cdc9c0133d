// The kernels DenseNet adds to the shared GEMMs (gfx950): the pre-activation BatchNorm -> ReLU that every consumer applies with its own
// affine to a channel PREFIX of the block's concat buffer, its backward that adds into a channel prefix of the block's gradient buffer,
// both again with the 2x2 / 2 average pool of a transition folded in, and a strided slice copy.  All of it is HBM-bound element work on
// NHWC rows, 16-byte (8-channel) vectors per lane, grid-strided.
//
// One kernel text per operation, instantiated for the two storages (bf16; PAIR: hi + lo planes of the reference-precision mode).  The
// arithmetic is fp32 on the joined value: a = fmaf(s, x, t) (one rounding, so the sign of a is the sign of the exact s x + t), then
// ReLU, then the hardware round-to-nearest-even split into the storage.  A NaN stays a NaN (torch.relu's rule), -0 becomes +0.
// Sign tensors: 1 bit per element of the dense [rows][C] operand, byte (r * C + c) / 8, bit c & 7 (the convention of the GEMM
// epilogues); C % 32 == 0 lets four neighbouring lanes of a row gather their bytes into one 32-bit store.
#include "rart_common.h"
#include "rart_bf16_helpers.h"

namespace {
using namespace rart_bf16;
constexpr int kBlock = 256;

__device__ __forceinline__ void load_f8(const float* __restrict__ p, float* f) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
// eight values into the storage at element i: bf16, or (PAIR) hi = bf16(v) and lo = bf16(v - hi), hardware round-to-nearest-even.  Where hi
// is infinite (v is, or rounds there) lo is zero, not the NaN of inf - inf: the joined value stays the infinity.  A NaN stays a NaN.
template <bool PAIR>
__device__ __forceinline__ void store8(uint16_t* __restrict__ h, uint16_t* __restrict__ l, size_t i, const float* v) {
  uint4 hi, lo;
  split8(v, hi, lo);
  *reinterpret_cast<uint4*>(h + i) = hi;
  if (PAIR) {
    float hf[8], r[8];
    unpack8(hi, hf);
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (fabsf(hf[j]) == INFINITY) ? 0.f : v[j] - hf[j];
    uint4 unused;
    split8(r, lo, unused);
    *reinterpret_cast<uint4*>(l + i) = lo;
  }
}
// relu(s x + t) of eight channels, in place
__device__ __forceinline__ void affine_relu8(float* x, const float* s, const float* t) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a = fmaf(s[j], x[j], t[j]);
    x[j] = (a <= 0.f) ? 0.f : a;
  }
}
// bit j = value j > 0
__device__ __forceinline__ uint32_t positive_byte(const float* v) {
  uint32_t b = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) b |= (v[j] > 0.f ? 1u : 0u) << j;
  return b;
}
// eight values as the storage will hold them (hi plane), for the sign of the STORED value
__device__ __forceinline__ uint32_t stored_positive_byte(const float* v) {
  uint4 hi, lo;
  split8(v, hi, lo);
  float h[8];
  unpack8(hi, h);
  return positive_byte(h);
}
// the sign bytes of the four lanes 4q .. 4q + 3 (consecutive byte indices i .. i + 3, i % 4 == 0 at lane 4q) as one 32-bit store.  Every
// lane of the wave calls this (the shuffles read the neighbours); `valid` lanes come in whole quads because the item count is a
// multiple of 4.
__device__ __forceinline__ void store_sign_quad(uint8_t* __restrict__ sign, size_t i, uint32_t byte, bool valid) {
  const uint32_t b1 = __shfl_down(byte, 1, 64), b2 = __shfl_down(byte, 2, 64), b3 = __shfl_down(byte, 3, 64);
  if (valid && (threadIdx.x & 3) == 0) *reinterpret_cast<uint32_t*>(sign + i) = byte | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

// y[r][c] = relu(s[c] x[r][c] + t[c]), c < C; x rows ld_x apart, y dense; item = (row, 8 channels)
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_dn_preact(const uint16_t* __restrict__ x_hi, const uint16_t* __restrict__ x_lo, int ld_x,
                                                      const float* __restrict__ s, const float* __restrict__ t,
                                                      uint16_t* __restrict__ y_hi, uint16_t* __restrict__ y_lo,
                                                      uint8_t* __restrict__ sign, size_t rows, int c8) {
  const size_t total = rows * c8, step = (size_t)gridDim.x * kBlock;
  const size_t rounds = (total + step - 1) / step;               // every lane runs every round: the sign gather shuffles across lanes
  size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  for (size_t k = 0; k < rounds; ++k, i += step) {
    const bool valid = i < total;
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (valid) {
      const size_t r = i / c8;
      const int v = (int)(i - r * c8);
      float sv[8], tv[8];
      load_f8(s + v * 8, sv);
      load_f8(t + v * 8, tv);
      ld8<PAIR>(x_hi, x_lo, r * ld_x + (size_t)v * 8, f);
      affine_relu8(f, sv, tv);
      store8<PAIR>(y_hi, y_lo, i * 8, f);
    }
    if (sign) store_sign_quad(sign, i, stored_positive_byte(f), valid);
  }
}

// the transition's form: y[b][oy][ox][c] = mean over the 2x2 window of relu(s x + t); sign bits of the four activated values at full
// resolution ([n][h][w][C / 8]); item = (output pixel, 8 channels)
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_dn_preact_pool2(const uint16_t* __restrict__ x_hi, const uint16_t* __restrict__ x_lo, int ld_x,
                                                            const float* __restrict__ s, const float* __restrict__ t,
                                                            uint16_t* __restrict__ y_hi, uint16_t* __restrict__ y_lo,
                                                            uint8_t* __restrict__ sign, int n, int h, int w, int c8) {
  const int oh = h / 2, ow = w / 2;
  const size_t total = (size_t)n * oh * ow * c8, step = (size_t)gridDim.x * kBlock;
  const size_t rounds = (total + step - 1) / step;
  size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  for (size_t k = 0; k < rounds; ++k, i += step) {
    const bool valid = i < total;
    float a[4][8];
    size_t pix[4] = {0, 0, 0, 0};
    int v = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 8; ++j) a[q][j] = 0.f;
    if (valid) {
      size_t p = i / c8;
      v = (int)(i - p * c8);
      const int ox = (int)(p % ow);
      p /= ow;
      const int oy = (int)(p % oh);
      const size_t img = p / oh;
      float sv[8], tv[8];
      load_f8(s + v * 8, sv);
      load_f8(t + v * 8, tv);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        pix[q] = (img * h + (2 * oy + (q >> 1))) * w + (2 * ox + (q & 1));
        ld8<PAIR>(x_hi, x_lo, pix[q] * ld_x + (size_t)v * 8, a[q]);
        affine_relu8(a[q], sv, tv);
      }
      float m[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) m[j] = ((a[0][j] + a[1][j]) + (a[2][j] + a[3][j])) * 0.25f;
      store8<PAIR>(y_hi, y_lo, i * 8, m);
    }
    if (sign) {
#pragma unroll
      for (int q = 0; q < 4; ++q) store_sign_quad(sign, pix[q] * c8 + v, positive_byte(a[q]), valid);
    }
  }
}

// g[r][c] (=|+=) bit[r][c] * s[c] * d[r'][c], c < C; g rows ld_g apart, channels >= C untouched; d dense.  POOL: r = full-resolution
// pixel (b, y, x), r' = its pooled pixel (b, y / 2, x / 2) and the value is d / 4; else r' = r.  s may be null (= 1).
template <bool PAIR, bool POOL>
__global__ __launch_bounds__(kBlock) void k_dn_preact_bwd(const uint16_t* __restrict__ d_hi, const uint16_t* __restrict__ d_lo,
                                                          const uint8_t* __restrict__ bits, const float* __restrict__ s,
                                                          uint16_t* __restrict__ g_hi, uint16_t* __restrict__ g_lo, int ld_g,
                                                          int accumulate, size_t rows, int h, int w, int c8) {
  const size_t total = rows * c8;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
    const size_t r = i / c8;
    const int v = (int)(i - r * c8);
    size_t rd = r;
    if (POOL) {
      const int x = (int)(r % w);
      const size_t t = r / w;
      const int y = (int)(t % h);
      rd = ((t / h) * (h / 2) + y / 2) * (w / 2) + x / 2;
    }
    float f[8], sv[8];
    ld8<PAIR>(d_hi, d_lo, (rd * c8 + v) * 8, f);
    const uint32_t b = bits[i];
    if (s) {
      load_f8(s + v * 8, sv);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] *= sv[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (POOL) f[j] *= 0.25f;
      if (!((b >> j) & 1u)) f[j] = 0.f;
    }
    const size_t at = r * ld_g + (size_t)v * 8;
    if (accumulate) {
      float o[8];
      ld8<PAIR>(g_hi, g_lo, at, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += o[j];
    }
    store8<PAIR>(g_hi, g_lo, at, f);
  }
}

// dst[r][c] = src[r][c], c < C, rows ld_src / ld_dst apart: a channel slice in or out of a concat buffer (bit copy of each plane)
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_dn_copy(const uint16_t* __restrict__ s_hi, const uint16_t* __restrict__ s_lo, int ld_src,
                                                    uint16_t* __restrict__ d_hi, uint16_t* __restrict__ d_lo, int ld_dst, size_t rows, int c8) {
  const size_t total = rows * c8;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
    const size_t r = i / c8;
    const size_t v = i - r * c8;
    *reinterpret_cast<uint4*>(d_hi + r * ld_dst + v * 8) = *reinterpret_cast<const uint4*>(s_hi + r * ld_src + v * 8);
    if (PAIR) *reinterpret_cast<uint4*>(d_lo + r * ld_dst + v * 8) = *reinterpret_cast<const uint4*>(s_lo + r * ld_src + v * 8);
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool al4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// the checks every entry shares: a strided tensor of `rows` rows, C of ld channels
#define DN_CHECK_SHAPE(what, rows, c, ld)                                                                                       \
  RART_CHECK_ARG((rows) > 0 && (rows) < (1ll << 31), what ": the row count must be in 1 .. 2^31 - 1");                          \
  RART_CHECK_ARG((c) >= 32 && (c) % 32 == 0, what ": the channel count must be a positive multiple of 32");                     \
  RART_CHECK_ARG((ld) >= (c) && (ld) % 8 == 0, what ": a row stride must cover the channels and keep 16-byte alignment (ld %% 8 == 0)")

template <bool PAIR>
int launch_preact(const void* x_hi, const void* x_lo, int ld_x, const float* s, const float* t, void* y_hi, void* y_lo, void* sign,
                  long long rows, int c, rart_stream_t stream) {
  RART_CHECK_ARG(x_hi && s && t && y_hi && (!PAIR || (x_lo && y_lo)), "rart_dn_preact: null tensor pointer");
  DN_CHECK_SHAPE("rart_dn_preact", rows, c, ld_x);
  RART_CHECK_ARG(al16(x_hi) && al16(x_lo) && al16(y_hi) && al16(y_lo) && al16(s) && al16(t) && al4(sign),
                 "rart_dn_preact: tensors must be 16-byte aligned (the sign tensor 4-byte)");
  hipLaunchKernelGGL(k_dn_preact<PAIR>, dim3(rart_grid_wide((size_t)rows * (c / 8))), dim3(kBlock), 0, (hipStream_t)stream,
                     (const uint16_t*)x_hi, (const uint16_t*)x_lo, ld_x, s, t, (uint16_t*)y_hi, (uint16_t*)y_lo, (uint8_t*)sign, (size_t)rows,
                     c / 8);
  RART_CHECK_LAUNCH("rart_dn_preact");
  return RART_OK;
}

template <bool PAIR>
int launch_preact_pool2(const void* x_hi, const void* x_lo, int ld_x, const float* s, const float* t, void* y_hi, void* y_lo, void* sign,
                        int n, int h, int w, int c, rart_stream_t stream) {
  RART_CHECK_ARG(x_hi && s && t && y_hi && (!PAIR || (x_lo && y_lo)), "rart_dn_preact_pool2: null tensor pointer");
  RART_CHECK_ARG(n > 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0, "rart_dn_preact_pool2: n > 0, h and w positive and even");
  DN_CHECK_SHAPE("rart_dn_preact_pool2", (long long)n * h * w, c, ld_x);
  RART_CHECK_ARG(al16(x_hi) && al16(x_lo) && al16(y_hi) && al16(y_lo) && al16(s) && al16(t) && al4(sign),
                 "rart_dn_preact_pool2: tensors must be 16-byte aligned (the sign tensor 4-byte)");
  hipLaunchKernelGGL(k_dn_preact_pool2<PAIR>, dim3(rart_grid_wide((size_t)n * (h / 2) * (w / 2) * (c / 8))), dim3(kBlock), 0,
                     (hipStream_t)stream, (const uint16_t*)x_hi, (const uint16_t*)x_lo, ld_x, s, t, (uint16_t*)y_hi, (uint16_t*)y_lo,
                     (uint8_t*)sign, n, h, w, c / 8);
  RART_CHECK_LAUNCH("rart_dn_preact_pool2");
  return RART_OK;
}

template <bool PAIR, bool POOL>
int launch_preact_bwd(const char* what, const void* d_hi, const void* d_lo, const void* bits, const float* s, void* g_hi, void* g_lo, int ld_g,
                      int accumulate, long long rows, int h, int w, int c, rart_stream_t stream) {
  RART_CHECK_ARG(d_hi && bits && g_hi && (!PAIR || (d_lo && g_lo)), "%s: null tensor pointer", what);
  RART_CHECK_ARG(rows > 0 && rows < (1ll << 31), "%s: the row count must be in 1 .. 2^31 - 1", what);
  RART_CHECK_ARG(c >= 32 && c % 32 == 0, "%s: the channel count must be a positive multiple of 32", what);
  RART_CHECK_ARG(ld_g >= c && ld_g % 8 == 0, "%s: ld_g must cover the channels and keep 16-byte alignment (ld_g %% 8 == 0)", what);
  RART_CHECK_ARG(accumulate == 0 || accumulate == 1, "%s: accumulate is 0 (write) or 1 (add)", what);
  RART_CHECK_ARG(al16(d_hi) && al16(d_lo) && al16(g_hi) && al16(g_lo) && al16(s), "%s: tensors must be 16-byte aligned", what);
  hipLaunchKernelGGL((k_dn_preact_bwd<PAIR, POOL>), dim3(rart_grid_wide((size_t)rows * (c / 8))), dim3(kBlock), 0, (hipStream_t)stream,
                     (const uint16_t*)d_hi, (const uint16_t*)d_lo, (const uint8_t*)bits, s, (uint16_t*)g_hi, (uint16_t*)g_lo, ld_g, accumulate,
                     (size_t)rows, h, w, c / 8);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}

template <bool PAIR>
int launch_pool2_bwd(const char* what, const void* d_hi, const void* d_lo, const void* bits, const float* s, void* g_hi, void* g_lo, int ld_g,
                     int accumulate, int n, int h, int w, int c, rart_stream_t stream) {
  RART_CHECK_ARG(n > 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0, "%s: n > 0, h and w positive and even", what);
  return launch_preact_bwd<PAIR, true>(what, d_hi, d_lo, bits, s, g_hi, g_lo, ld_g, accumulate, (long long)n * h * w, h, w, c, stream);
}

template <bool PAIR>
int launch_copy(const void* s_hi, const void* s_lo, int ld_src, void* d_hi, void* d_lo, int ld_dst, long long rows, int c, rart_stream_t stream) {
  RART_CHECK_ARG(s_hi && d_hi && (!PAIR || (s_lo && d_lo)), "rart_dn_copy: null tensor pointer");
  DN_CHECK_SHAPE("rart_dn_copy", rows, c, ld_src);
  RART_CHECK_ARG(ld_dst >= c && ld_dst % 8 == 0, "rart_dn_copy: ld_dst must cover the channels and keep 16-byte alignment (ld_dst %% 8 == 0)");
  RART_CHECK_ARG(al16(s_hi) && al16(s_lo) && al16(d_hi) && al16(d_lo), "rart_dn_copy: tensors must be 16-byte aligned");
  hipLaunchKernelGGL(k_dn_copy<PAIR>, dim3(rart_grid_wide((size_t)rows * (c / 8))), dim3(kBlock), 0, (hipStream_t)stream, (const uint16_t*)s_hi,
                     (const uint16_t*)s_lo, ld_src, (uint16_t*)d_hi, (uint16_t*)d_lo, ld_dst, (size_t)rows, c / 8);
  RART_CHECK_LAUNCH("rart_dn_copy");
  return RART_OK;
}
}  // namespace

extern "C" {

int rart_dn_preact_bf16(const void* x, int ld_x, const float* s, const float* t, void* y, void* sign_out, long long rows, int c,
                        rart_stream_t stream) {
  return launch_preact<false>(x, nullptr, ld_x, s, t, y, nullptr, sign_out, rows, c, stream);
}
int rart_dn_preact_pair(const void* x_hi, const void* x_lo, int ld_x, const float* s, const float* t, void* y_hi, void* y_lo, void* sign_out,
                        long long rows, int c, rart_stream_t stream) {
  return launch_preact<true>(x_hi, x_lo, ld_x, s, t, y_hi, y_lo, sign_out, rows, c, stream);
}

int rart_dn_preact_bwd_bf16(const void* d, const void* bits, const float* s, void* g, int ld_g, int accumulate, long long rows, int c,
                            rart_stream_t stream) {
  return launch_preact_bwd<false, false>("rart_dn_preact_bwd_bf16", d, nullptr, bits, s, g, nullptr, ld_g, accumulate, rows, 0, 0, c, stream);
}
int rart_dn_preact_bwd_pair(const void* d_hi, const void* d_lo, const void* bits, const float* s, void* g_hi, void* g_lo, int ld_g, int accumulate,
                            long long rows, int c, rart_stream_t stream) {
  return launch_preact_bwd<true, false>("rart_dn_preact_bwd_pair", d_hi, d_lo, bits, s, g_hi, g_lo, ld_g, accumulate, rows, 0, 0, c, stream);
}

int rart_dn_preact_pool2_bf16(const void* x, int ld_x, const float* s, const float* t, void* y, void* sign_out, int n, int h, int w, int c,
                              rart_stream_t stream) {
  return launch_preact_pool2<false>(x, nullptr, ld_x, s, t, y, nullptr, sign_out, n, h, w, c, stream);
}
int rart_dn_preact_pool2_pair(const void* x_hi, const void* x_lo, int ld_x, const float* s, const float* t, void* y_hi, void* y_lo,
                              void* sign_out, int n, int h, int w, int c, rart_stream_t stream) {
  return launch_preact_pool2<true>(x_hi, x_lo, ld_x, s, t, y_hi, y_lo, sign_out, n, h, w, c, stream);
}

int rart_dn_preact_pool2_bwd_bf16(const void* d, const void* bits, const float* s, void* g, int ld_g, int accumulate, int n, int h, int w,
                                  int c, rart_stream_t stream) {
  return launch_pool2_bwd<false>("rart_dn_preact_pool2_bwd_bf16", d, nullptr, bits, s, g, nullptr, ld_g, accumulate, n, h, w, c, stream);
}
int rart_dn_preact_pool2_bwd_pair(const void* d_hi, const void* d_lo, const void* bits, const float* s, void* g_hi, void* g_lo, int ld_g,
                                  int accumulate, int n, int h, int w, int c, rart_stream_t stream) {
  return launch_pool2_bwd<true>("rart_dn_preact_pool2_bwd_pair", d_hi, d_lo, bits, s, g_hi, g_lo, ld_g, accumulate, n, h, w, c, stream);
}

int rart_dn_copy_bf16(const void* src, int ld_src, void* dst, int ld_dst, long long rows, int c, rart_stream_t stream) {
  return launch_copy<false>(src, nullptr, ld_src, dst, nullptr, ld_dst, rows, c, stream);
}
int rart_dn_copy_pair(const void* src_hi, const void* src_lo, int ld_src, void* dst_hi, void* dst_lo, int ld_dst, long long rows, int c,
                      rart_stream_t stream) {
  return launch_copy<true>(src_hi, src_lo, ld_src, dst_hi, dst_lo, ld_dst, rows, c, stream);
}

}  // extern "C"
