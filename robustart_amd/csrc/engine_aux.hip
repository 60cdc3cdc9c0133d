// Non-GEMM kernels of the ResNet-50 engines (gfx950): input preparation (normalise + bf16 hi/lo split + spatial/channel padding for
// the 7x7 stem), 3x3/2 max-pool forward and backward (+ReLU mask), global average pool forward/backward, the stem's col2im (backward
// to the fp32 image), an fp32 -> padded row converter and the small-M GEMM of the classifier head.  All HBM-bound elementwise/gather
// work on NHWC tensors, 16-byte (8-channel) vectors per lane.
//
// One kernel text per operation, instantiated for the two storages: bf16, and the PAIR of bf16 planes of the reference-precision mode.
// The reference runs fp32 everywhere (RobustART/noise/utils/adv/attack.py:20-23, Attacks/autoattack/autopgd_base.py:271-289: fp32
// logits and gradients); the "bf16x3" mode keeps every activation / gradient as value = hi + lo with hi = bf16(v), lo = bf16(v - hi)
// -- 16 significand bits in the bytes of one fp32 -- so that the MFMA kernels can form x.w as x_hi.w_hi + x_hi.w_lo + x_lo.w_hi with
// fp32 accumulation (conv_igemm.hip, flag 32).  hi + lo is exact in fp32 (two 8-bit significands, |lo| <= half an ulp of hi), so a
// pair instance unpacks to fp32, computes what the bf16 instance computes, and splits again: the storages differ in load8 / store8
// below and in where the two backward kernels take their ReLU mask from, nowhere else.
#include "rart_common.h"
#include "rart_bf16_helpers.h"

namespace {
using namespace rart_bf16;
constexpr int kBlock = 256;

// ---- the 8 channels at vector index i as fp32.  PAIR: p is the hi plane and the lo plane lies lo_off vectors behind it; bf16 ignores
//      lo_off.  Both stores round with the software f2bf (pack8; hi = f2bf(v), lo = f2bf(v - hi)), NOT with the hardware convert of
//      split8 / st8, which makes other bits of a NaN (rart_row_norm.h has the two side by side).  The kernels take their lo offsets
//      LAST: a bf16 instance then finds the arguments it uses where a kernel without them would, and compiles to the same instructions
template <bool PAIR>
__device__ __forceinline__ void load8(const uint4* __restrict__ p, size_t lo_off, size_t i, float* f) {
  if (!PAIR) {
    unpack8(p[i], f);
    return;
  }
  const uint4 a = p[i], b = p[i + lo_off];
  const uint32_t wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = bf2f(wa[j] & 0xFFFFu) + bf2f(wb[j] & 0xFFFFu);
    f[2 * j + 1] = bf2f(wa[j] >> 16) + bf2f(wb[j] >> 16);
  }
}
template <bool PAIR>
__device__ __forceinline__ void store8(uint4* __restrict__ p, size_t lo_off, size_t i, const float* f) {
  if (!PAIR) {
    p[i] = pack8(f);
    return;
  }
  uint32_t h[8], l[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    h[j] = f2bf(f[j]);
    l[j] = f2bf(f[j] - bf2f(h[j]));
  }
  p[i] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
  p[i + lo_off] = make_uint4(l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16));
}

#pragma clang fp contract(off)   // op-by-op rounding: the fused stem forward (stem_fused.hip) restates this arithmetic
// src: fp32 NCHW in [0,1] (SRC_U8 = false) or uint8 NHWC (SRC_U8 = true).
// dst hi/lo: bf16 [n][h+8][w+8][4], image at offset (3,3), zero elsewhere; v = (x - mean)/std,
// hi = bf16(v), lo = bf16(v - hi): hi + lo carries ~16 mantissa bits so eps-sized PGD steps survive.
template <bool SRC_U8>
__global__ __launch_bounds__(kBlock) void k_prep_input(const void* __restrict__ src, uint2* __restrict__ hi,
                                                       uint2* __restrict__ lo, int n, int h, int w, RartNorm3 nm) {
  const int ph = h + 8, pw = w + 8;
  const size_t total = (size_t)n * ph * pw;
  for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < total; p += (size_t)gridDim.x * kBlock) {
    const int px = (int)(p % pw), py = (int)((p / pw) % ph);
    const int img = (int)(p / ((size_t)pw * ph));
    const int x = px - 3, y = py - 3;
    uint16_t hv[4] = {0, 0, 0, 0}, lv[4] = {0, 0, 0, 0};
    if ((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v01;
        if (SRC_U8)
          v01 = (float)((const uint8_t*)src)[(((size_t)img * h + y) * w + x) * 3 + c] * (1.0f / 255.0f);
        else
          v01 = ((const float*)src)[(((size_t)img * 3 + c) * h + y) * w + x];
        const float v = (v01 - nm.mean[c]) * nm.istd[c];
        hv[c] = f2bf(v);
        lv[c] = f2bf(v - bf2f(hv[c]));
      }
    }
    hi[p] = make_uint2(hv[0] | ((uint32_t)hv[1] << 16), hv[2] | ((uint32_t)hv[3] << 16));
    lo[p] = make_uint2(lv[0] | ((uint32_t)lv[1] << 16), lv[2] | ((uint32_t)lv[3] << 16));
  }
}

#pragma clang fp contract(fast)
// 3x3 stride-2 pad-1 max pool, NHWC, one thread per (output pixel, 8 channels).  Also records, per
// channel, WHICH of the 9 window positions (ky*3+kx) holds the first maximum in scan order (PyTorch's
// argmax rule) as one byte, so the backward is a <= 4-window gather instead of a 36-tap search.
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_maxpool_fwd(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                        uint2* __restrict__ arg, uint8_t* __restrict__ sign, int n, int h,
                                                        int w, int c8, size_t in_lo, size_t out_lo) {
  const int oh = h / 2, ow = w / 2;
  const size_t total = (size_t)n * oh * ow * c8;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
    const int c = (int)(i % c8);
    size_t t = i / c8;
    const int ox = (int)(t % ow);
    t /= ow;
    const int oy = (int)(t % oh);
    const int img = (int)(t / oh);
    float m[8];
    uint32_t code[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { m[j] = -INFINITY; code[j] = 0; }
    for (int ky = 0; ky < 3; ++ky) {
      const int y = oy * 2 - 1 + ky;
      if ((unsigned)y >= (unsigned)h) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int x = ox * 2 - 1 + kx;
        if ((unsigned)x >= (unsigned)w) continue;
        float f[8];
        load8<PAIR>(in, in_lo, (((size_t)img * h + y) * w + x) * c8 + c, f);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (f[j] > m[j]) { m[j] = f[j]; code[j] = (uint32_t)(ky * 3 + kx); }
      }
    }
    store8<PAIR>(out, out_lo, i, m);
    // code 15 = the window maximum is <= 0: behind a ReLU its gradient is dead, so the fused stem backward
    // (stem_fused.hip) needs no second look at y; it never equals a window position, k_maxpool_bwd is unaffected
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (!(m[j] > 0.f)) code[j] = 15u;
    if (sign) {       // 1 bit per channel: pooled value > 0 (the ReLU mask of the first block's input)
      uint32_t sb = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) sb |= (m[j] > 0.f ? 1u : 0u) << j;
      sign[i] = (uint8_t)sb;
    }
    if (arg)
      arg[i] = make_uint2(code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24),
                          code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24));
  }
}

// backward of the pool fused with the ReLU mask of its input y (= relu(stem conv)):
// dz[h,w,c] = (y > 0) * sum over the <= 4 windows containing (h,w) whose recorded argmax is (h,w).
// bf16 reads y for the mask.  PAIR takes no y: code 15 already marks the windows whose maximum is <= 0 and a window's argmax position
// holds that maximum, so the codes alone decide.
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_maxpool_bwd(const uint4* __restrict__ y, const uint2* __restrict__ arg,
                                                        const uint4* __restrict__ dpool, uint4* __restrict__ dz, int n,
                                                        int h, int w, int c8, size_t dpool_lo, size_t dz_lo) {
  const int oh = h / 2, ow = w / 2;
  const size_t total = (size_t)n * h * w * c8;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
    const int c = (int)(i % c8);
    size_t t = i / c8;
    const int x = (int)(t % w);
    t /= w;
    const int yy = (int)(t % h);
    const int img = (int)(t / h);
    float self[8], g[8];
    if (!PAIR) unpack8(y[i], self);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = 0.f;
    // windows o with 2o-1 <= pos <= 2o+1: o = pos/2 (always) and o = (pos+1)/2 when pos is odd
    const int oy0 = yy >> 1, ox0 = x >> 1;
    const int nys = (yy & 1) ? 2 : 1, nxs = (x & 1) ? 2 : 1;
    for (int a = 0; a < nys; ++a) {
      const int oy = oy0 + a;
      if (oy >= oh) continue;
      const uint32_t ky = (uint32_t)(yy - (2 * oy - 1));
      for (int b = 0; b < nxs; ++b) {
        const int ox = ox0 + b;
        if (ox >= ow) continue;
        const uint32_t mine = ky * 3 + (uint32_t)(x - (2 * ox - 1));
        const size_t wi = (((size_t)img * oh + oy) * ow + ox) * c8 + c;
        const uint2 cd = arg[wi];
        float dp[8];
        load8<PAIR>(dpool, dpool_lo, wi, dp);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t cj = ((j < 4 ? cd.x : cd.y) >> (8 * (j & 3))) & 0xFFu;
          if (cj == mine) g[j] += dp[j];
        }
      }
    }
    if (!PAIR) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (!(self[j] > 0.f)) g[j] = 0.f;
    }
    store8<PAIR>(dz, dz_lo, i, g);
  }
}

// global average pool [n][hw][c] -> [n][c], fp32 accumulation in position order
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_avgpool_fwd(const uint4* __restrict__ in, uint4* __restrict__ out, int n,
                                                        int hw, int c8, size_t in_lo, size_t out_lo) {
  const size_t total = (size_t)n * c8;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
    const int c = (int)(i % c8), img = (int)(i / c8);
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
    for (int p = 0; p < hw; ++p) {
      float f[8];
      load8<PAIR>(in, in_lo, ((size_t)img * hw + p) * c8 + c, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += f[j];
    }
    const float inv = 1.0f / (float)hw;
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] *= inv;
    store8<PAIR>(out, out_lo, i, s);
  }
}

// dz[n][p][c] = (y[n][p][c] > 0) ? dpool[n][c] / hw : 0.  bf16: `mask` is y itself, one 16-byte vector per item.  PAIR: `mask` is the
// sign bytes the forward kept, one byte per item (bit j = channel j > 0)
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_avgpool_bwd(const void* __restrict__ mask, const uint4* __restrict__ dpool,
                                                        uint4* __restrict__ dz, int n, int hw, int c8, size_t dpool_lo,
                                                        size_t dz_lo) {
  const size_t total = (size_t)n * hw * c8;
  const float inv = 1.0f / (float)hw;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
    const int c = (int)(i % c8), img = (int)(i / ((size_t)hw * c8));
    float f[8], d[8];
    uint32_t sb = 0;
    if (!PAIR) unpack8(static_cast<const uint4*>(mask)[i], f);
    load8<PAIR>(dpool, dpool_lo, (size_t)img * c8 + c, d);
    if (PAIR) sb = static_cast<const uint8_t*>(mask)[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = (PAIR ? ((sb >> j) & 1u) != 0 : f[j] > 0.f) ? d[j] * inv : 0.f;
    store8<PAIR>(dz, dz_lo, i, d);
  }
}

// fp32 rows -> zero-padded bf16 or pair rows (dlogits for the fc backward); dst_lo in elements
template <bool PAIR>
__global__ __launch_bounds__(kBlock) void k_f32_to_rows(const float* __restrict__ src, uint16_t* __restrict__ dst, int rows,
                                                        int cols, int dst_cols, size_t dst_lo) {
  const size_t total = (size_t)rows * dst_cols;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
    const int c = (int)(i % dst_cols);
    const size_t r = i / dst_cols;
    const float v = c < cols ? src[r * cols + c] : 0.f;
    const uint32_t h = f2bf(v);
    dst[i] = (uint16_t)h;
    if (PAIR) dst[i + dst_lo] = (uint16_t)f2bf(v - bf2f(h));
  }
}

// Stem backward: patches[n][oh][ow][pc = 152] (T = uint16_t: bf16, or float; column (r*7+s)*3+c, 147 rounded up to 8) -> grad fp32 NCHW
// dx[n][c][h][w] = istd[c] * sum_{r,s: (h+3-r), (w+3-s) even, p,q in range} patches[n][p][q][(r*7+s)*3+c]
// One workgroup of NT threads = a TH x TW tile of image pixels: the (TH/2+3) x (TW/2+3) patch rows that reach it (304 or 608 B each)
// are staged in LDS with coalesced 16-byte loads, then every pixel gathers its <= 16 overlapping taps from LDS (the first
// version issued 48 scattered 2-byte global loads per pixel: 0.79 ms per launch at B = 256, 6.5 % of a gradient evaluation).
constexpr int C2I_PC = 152;
__device__ __forceinline__ float c2i_val(uint16_t v) { return bf2f(v); }
__device__ __forceinline__ float c2i_val(float v) { return v; }
// the staged rows are a static array where that may be (64 KB), else dynamic LDS
template <typename T>
constexpr bool c2i_static_lds(int th, int tw) { return (th / 2 + 3) * (tw / 2 + 3) * C2I_PC * sizeof(T) <= 64 * 1024; }
template <typename T, int TH, int TW, int NT>
__global__ __launch_bounds__(NT) void k_stem_col2im(const T* __restrict__ patches, float* __restrict__ grad, int n, int h, int w,
                                                    int pc, RartIstd3 is) {
  constexpr int PH = TH / 2 + 3, PW = TW / 2 + 3;
  T* sp;
  if constexpr (c2i_static_lds<T>(TH, TW)) {                          // bf16: 63 536 B
    __shared__ __attribute__((aligned(16))) T tile[PH * PW * C2I_PC];
    sp = tile;
  } else {                                                            // fp32: 127 072 B
    extern __shared__ __attribute__((aligned(16))) unsigned char c2i_lds[];
    sp = reinterpret_cast<T*>(c2i_lds);
  }
  const int oh = h / 2, ow = w / 2;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, img = blockIdx.z;
  const int p0 = y0 / 2 - 1, q0 = x0 / 2 - 1;                       // first patch row / column that reaches the tile
  constexpr int EV = 16 / sizeof(T), VEC = C2I_PC / EV;              // elements per 16-byte vector, vectors per patch row (19 or 38)
  constexpr int FILL_UNROLL = sizeof(T) == 4 ? 4 : 1;                // fp32: many loads in flight per CU; bf16 measured 8 % slower unrolled
  // pc stays a run-time factor: folded in as 152 the address becomes a longer dependent chain (bf16 +1.7 .. 3.8 %, fp32 +2.1 %)
#pragma unroll FILL_UNROLL
  for (int i = threadIdx.x; i < PH * PW * VEC; i += NT) {
    const int v = i % VEC, pos = i / VEC;
    const int pp = p0 + pos / PW, qq = q0 + pos % PW;
    uint4 val = make_uint4(0, 0, 0, 0);
    if ((unsigned)pp < (unsigned)oh && (unsigned)qq < (unsigned)ow)
      val = *reinterpret_cast<const uint4*>(patches + (((size_t)img * oh + pp) * ow + qq) * pc + v * EV);
    *reinterpret_cast<uint4*>(sp + (size_t)pos * C2I_PC + v * EV) = val;
  }
  __syncthreads();
  const size_t plane = (size_t)h * w;
  for (int i = threadIdx.x; i < TH * TW; i += NT) {
    const int x = x0 + i % TW, y = y0 + i / TW;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    for (int r = (y + 3) & 1; r < 7; r += 2) {
      const int pp = (y + 3 - r) >> 1;                                // same parity by construction; negative near the top edge
      if (y + 3 - r < 0 || pp >= oh) continue;
      for (int sft = (x + 3) & 1; sft < 7; sft += 2) {
        const int qq = (x + 3 - sft) >> 1;
        if (x + 3 - sft < 0 || qq >= ow) continue;
        const T* pt = sp + ((size_t)(pp - p0) * PW + (qq - q0)) * C2I_PC + (r * 7 + sft) * 3;
        g0 += c2i_val(pt[0]);
        g1 += c2i_val(pt[1]);
        g2 += c2i_val(pt[2]);
      }
    }
    float* o = grad + (size_t)img * 3 * plane + (size_t)y * w + x;
    o[0] = g0 * is.v[0];
    o[plane] = g1 * is.v[1];
    o[2 * plane] = g2 * is.v[2];
  }
}

// ---- small-M GEMM: C[M][N] = A[M][K] . W[N][K]^T (+ bias) for the classifier head and its backward (M = the batch, 256) ------------------
// The implicit-GEMM kernel gives such a product 2 x 8 tiles of 128 x 128: 16 workgroups for 256 CUs, each walking the whole K (43 us for
// 1 GFLOP).  Here a workgroup owns ONE 32 x 32 output tile (8 x 32 = 256 of them for the head) and its four waves split K; the operands
// are used once per workgroup, so the MFMA fragments come straight from global memory (A is 1 MB, W 4 MB: L2 resident), 16 bytes per
// lane, and the four partial tiles are summed through LDS in a fixed order.
__global__ __launch_bounds__(kBlock) void k_gemm_small_m(const uint16_t* __restrict__ a, int lda, const uint16_t* __restrict__ wgt, int ldw,
                                                         const float* __restrict__ bias, void* __restrict__ out, int ldo, int out_f32,
                                                         int M, int N, int K) {
  __shared__ float red[4][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hh = lane >> 5;
  const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
  const int row_a = min(m0 + l31, M - 1), row_w = min(n0 + l31, N - 1);       // rows past the edge recompute the last one; never stored
  const int kq = K / 4;                                                        // host: K % 64 == 0
  const uint16_t* pa = a + (size_t)row_a * lda + wave * kq + hh * 8;
  const uint16_t* pw = wgt + (size_t)row_w * ldw + wave * kq + hh * 8;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k = 0; k < kq; k += 16) {
    const uint4 av = *reinterpret_cast<const uint4*>(pa + k), wv = *reinterpret_cast<const uint4*>(pw + k);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, wv), acc, 0, 0, 0);
  }
  // acc[r] = partial C[m0 + (r&3) + 8*(r>>2) + 4*hh][n0 + l31]
#pragma unroll
  for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = wave * 4 + q;
    const float v = ((red[0][r][lane] + red[1][r][lane]) + red[2][r][lane]) + red[3][r][lane];
    const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * hh, n = n0 + l31;
    if (m < M && n < N) {
      const float y = v + (bias ? bias[n] : 0.f);
      if (out_f32) reinterpret_cast<float*>(out)[(size_t)m * ldo + n] = y;
      else reinterpret_cast<uint16_t*>(out)[(size_t)m * ldo + n] = f2bf(y);
    }
  }
}

// ---- the launchers behind the _bf16 / _pair entries.  `what` is the entry's name; lo offsets arrive in ELEMENTS (the kernels take
//      vectors) and are looked at for PAIR alone: the bf16 entries pass 0
bool lo_ok(long long off) { return off > 0 && off % 8 == 0; }

template <bool PAIR>
int launch_maxpool(const void* in, long long in_lo, void* out, long long out_lo, void* argmax_out, void* sign_out, int n, int h, int w,
                   int c, rart_stream_t stream, const char* what) {
  RART_CHECK_ARG(in && out && n > 0 && h % 2 == 0 && w % 2 == 0 && c % 8 == 0 && (!PAIR || (lo_ok(in_lo) && lo_ok(out_lo))),
                 "%s: bad arguments", what);
  hipLaunchKernelGGL(k_maxpool_fwd<PAIR>, dim3(rart_grid_wide((size_t)n * (h / 2) * (w / 2) * (c / 8))), dim3(kBlock), 0,
                     (hipStream_t)stream, (const uint4*)in, (uint4*)out, (uint2*)argmax_out, (uint8_t*)sign_out, n, h, w, c / 8,
                     (size_t)in_lo / 8, (size_t)out_lo / 8);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}

template <bool PAIR>
int launch_maxpool_bwd(const void* y, const void* argmax, const void* dpool, long long dpool_lo, void* dz, long long dz_lo, int n, int h,
                       int w, int c, rart_stream_t stream, const char* what) {
  RART_CHECK_ARG((PAIR || y) && argmax && dpool && dz && n > 0 && h % 2 == 0 && w % 2 == 0 && c % 8 == 0 &&
                     (!PAIR || (lo_ok(dpool_lo) && lo_ok(dz_lo))),
                 "%s: bad arguments", what);
  hipLaunchKernelGGL(k_maxpool_bwd<PAIR>, dim3(rart_grid_wide((size_t)n * h * w * (c / 8))), dim3(kBlock), 0, (hipStream_t)stream,
                     (const uint4*)y, (const uint2*)argmax, (const uint4*)dpool, (uint4*)dz, n, h, w, c / 8, (size_t)dpool_lo / 8,
                     (size_t)dz_lo / 8);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}

template <bool PAIR>
int launch_avgpool(const void* in, long long in_lo, void* out, long long out_lo, int n, int hw, int c, rart_stream_t stream,
                   const char* what) {
  RART_CHECK_ARG(in && out && n > 0 && hw > 0 && c % 8 == 0 && (!PAIR || (lo_ok(in_lo) && lo_ok(out_lo))), "%s: bad arguments", what);
  hipLaunchKernelGGL(k_avgpool_fwd<PAIR>, dim3(rart_grid_wide((size_t)n * (c / 8))), dim3(kBlock), 0, (hipStream_t)stream,
                     (const uint4*)in, (uint4*)out, n, hw, c / 8, (size_t)in_lo / 8, (size_t)out_lo / 8);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}

template <bool PAIR>
int launch_avgpool_bwd(const void* mask, const void* dpool, long long dpool_lo, void* dz, long long dz_lo, int n, int hw, int c,
                       rart_stream_t stream, const char* what) {
  RART_CHECK_ARG(mask && dpool && dz && n > 0 && hw > 0 && c % 8 == 0 && (!PAIR || (lo_ok(dpool_lo) && lo_ok(dz_lo))),
                 "%s: bad arguments", what);
  hipLaunchKernelGGL(k_avgpool_bwd<PAIR>, dim3(rart_grid_wide((size_t)n * hw * (c / 8))), dim3(kBlock), 0, (hipStream_t)stream, mask,
                     (const uint4*)dpool, (uint4*)dz, n, hw, c / 8, (size_t)dpool_lo / 8, (size_t)dz_lo / 8);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}

template <bool PAIR>
int launch_f32_to_rows(const float* src, void* dst, long long dst_lo, int rows, int cols, int dst_cols, rart_stream_t stream,
                       const char* what) {
  RART_CHECK_ARG(src && dst && rows > 0 && cols > 0 && dst_cols >= cols && (!PAIR || dst_lo > 0), "%s: bad arguments", what);
  hipLaunchKernelGGL(k_f32_to_rows<PAIR>, dim3(rart_grid_wide((size_t)rows * dst_cols)), dim3(kBlock), 0, (hipStream_t)stream, src,
                     (uint16_t*)dst, rows, cols, dst_cols, (size_t)dst_lo);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}

// the entries check h, w and patch_cols, each with its own message
template <typename T, int TH, int TW, int NT>
int launch_col2im(const void* patches, float* grad, int n, int h, int w, const float* std_host, rart_stream_t stream, const char* what) {
  constexpr int LDS = c2i_static_lds<T>(TH, TW) ? 0 : (TH / 2 + 3) * (TW / 2 + 3) * C2I_PC * (int)sizeof(T);      // dynamic bytes
  if (h % TH || w % TW) return RART_ERR_INVALID;
  if (LDS && !rart_raise_dynamic_lds((const void*)k_stem_col2im<T, TH, TW, NT>, LDS, what)) return RART_ERR_HIP;
  hipLaunchKernelGGL((k_stem_col2im<T, TH, TW, NT>), dim3(w / TW, h / TH, n), dim3(NT), LDS, (hipStream_t)stream, (const T*)patches, grad,
                     n, h, w, C2I_PC, rart_istd3(std_host));
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}
}  // namespace

extern "C" {

int rart_engine_prep_input(const void* src, int src_is_u8, void* hi, void* lo, int n, int h, int w,
                           const float* mean_host, const float* std_host, rart_stream_t stream) {
  RART_CHECK_ARG(src && hi && lo && n > 0 && h > 0 && w > 0, "rart_engine_prep_input: bad arguments");
  const RartNorm3 nm = rart_norm3(mean_host, std_host);
  const size_t total = (size_t)n * (h + 8) * (w + 8);
  if (src_is_u8)
    hipLaunchKernelGGL(k_prep_input<true>, dim3(rart_grid_wide(total)), dim3(kBlock), 0, (hipStream_t)stream, src, (uint2*)hi,
                       (uint2*)lo, n, h, w, nm);
  else
    hipLaunchKernelGGL(k_prep_input<false>, dim3(rart_grid_wide(total)), dim3(kBlock), 0, (hipStream_t)stream, src,
                       (uint2*)hi, (uint2*)lo, n, h, w, nm);
  RART_CHECK_LAUNCH("rart_engine_prep_input");
  return RART_OK;
}

int rart_engine_maxpool_keep(const void* in, void* out, void* argmax_out, void* sign_out, int n, int h, int w, int c,
                             rart_stream_t stream) {
  return launch_maxpool<false>(in, 0, out, 0, argmax_out, sign_out, n, h, w, c, stream, "rart_engine_maxpool");
}

int rart_engine_maxpool(const void* in, void* out, void* argmax_out, int n, int h, int w, int c,
                        rart_stream_t stream) {
  return rart_engine_maxpool_keep(in, out, argmax_out, nullptr, n, h, w, c, stream);
}

int rart_engine_maxpool_pair(const void* in_hi, long long in_lo_off, void* out_hi, long long out_lo_off, void* argmax_out,
                             void* sign_out, int n, int h, int w, int c, rart_stream_t stream) {
  return launch_maxpool<true>(in_hi, in_lo_off, out_hi, out_lo_off, argmax_out, sign_out, n, h, w, c, stream,
                              "rart_engine_maxpool_pair");
}

int rart_engine_maxpool_bwd(const void* y, const void* argmax, const void* dpool, void* dz, int n, int h, int w, int c,
                            rart_stream_t stream) {
  return launch_maxpool_bwd<false>(y, argmax, dpool, 0, dz, 0, n, h, w, c, stream, "rart_engine_maxpool_bwd");
}

int rart_engine_maxpool_bwd_pair(const void* argmax, const void* dpool_hi, long long dpool_lo_off, void* dz_hi,
                                 long long dz_lo_off, int n, int h, int w, int c, rart_stream_t stream) {
  return launch_maxpool_bwd<true>(nullptr, argmax, dpool_hi, dpool_lo_off, dz_hi, dz_lo_off, n, h, w, c, stream,
                                  "rart_engine_maxpool_bwd_pair");
}

int rart_engine_avgpool(const void* in, void* out, int n, int hw, int c, rart_stream_t stream) {
  return launch_avgpool<false>(in, 0, out, 0, n, hw, c, stream, "rart_engine_avgpool");
}

int rart_engine_avgpool_pair(const void* in_hi, long long in_lo_off, void* out_hi, long long out_lo_off, int n, int hw, int c,
                             rart_stream_t stream) {
  return launch_avgpool<true>(in_hi, in_lo_off, out_hi, out_lo_off, n, hw, c, stream, "rart_engine_avgpool_pair");
}

int rart_engine_avgpool_bwd(const void* y, const void* dpool, void* dz, int n, int hw, int c, rart_stream_t stream) {
  return launch_avgpool_bwd<false>(y, dpool, 0, dz, 0, n, hw, c, stream, "rart_engine_avgpool_bwd");
}

int rart_engine_avgpool_bwd_pair(const void* y_sign_bits, const void* dpool_hi, long long dpool_lo_off, void* dz_hi,
                                 long long dz_lo_off, int n, int hw, int c, rart_stream_t stream) {
  return launch_avgpool_bwd<true>(y_sign_bits, dpool_hi, dpool_lo_off, dz_hi, dz_lo_off, n, hw, c, stream,
                                  "rart_engine_avgpool_bwd_pair");
}

// bf16 patches: 16 x 32 pixel tiles on 256 threads
int rart_engine_stem_col2im(const void* patches, float* grad, int n, int h, int w, int patch_cols,
                            const float* std_host, rart_stream_t stream) {
  RART_CHECK_ARG(patches && grad && n > 0 && n <= 65535 && h % 16 == 0 && w % 32 == 0 && patch_cols == C2I_PC,
                 "rart_engine_stem_col2im: h %% 16 == 0, w %% 32 == 0, patch_cols == 152 (147 rounded up to 8), n <= 65535");
  return launch_col2im<uint16_t, 16, 32, 256>(patches, grad, n, h, w, std_host, stream, "rart_engine_stem_col2im");
}

int rart_engine_stem_col2im_f32(const float* patches, float* grad, int n, int h, int w, int patch_cols, const float* std_host,
                                rart_stream_t stream) {
  RART_CHECK_ARG(patches && grad && n > 0 && n <= 65535 && h % 16 == 0 && w % 32 == 0 && patch_cols == C2I_PC,
                 "rart_engine_stem_col2im_f32: h %% 16 == 0, w %% 32 == 0, patch_cols == 152, n <= 65535");
  // 16 x 32 pixel tiles, 1 024 threads (measured at B = 256: 0.78 ms; 8 x 16 / 256 threads 1.29, 16 x 32 / 256 threads 1.86,
  // 8 x 32 / 512 0.84, 16 x 16 / 512 0.80: the fill phase wants many loads in flight per CU, the tile few halo re-reads)
  return launch_col2im<float, 16, 32, 1024>(patches, grad, n, h, w, std_host, stream, "rart_engine_stem_col2im_f32");
}

int rart_f32_to_bf16_rows(const float* src, void* dst, int rows, int cols, int dst_cols, rart_stream_t stream) {
  return launch_f32_to_rows<false>(src, dst, 0, rows, cols, dst_cols, stream, "rart_f32_to_bf16_rows");
}

int rart_f32_to_pair_rows(const float* src, void* dst_hi, long long dst_lo_off, int rows, int cols, int dst_cols,
                          rart_stream_t stream) {
  return launch_f32_to_rows<true>(src, dst_hi, dst_lo_off, rows, cols, dst_cols, stream, "rart_f32_to_pair_rows");
}

int rart_gemm_small_m_bf16(const void* a, int lda, const void* w, int ldw, const float* bias, void* out, int ldo, int out_is_f32, int m,
                           int n, int k, rart_stream_t stream) {
  RART_CHECK_ARG(a && w && out && m > 0 && n > 0 && k > 0 && k % 64 == 0 && lda >= k && ldw >= k && lda % 8 == 0 && ldw % 8 == 0 && ldo >= n,
                 "rart_gemm_small_m_bf16: k must be a multiple of 64, leading dimensions multiples of 8 and at least k (a, w) / n (out)");
  RART_CHECK_ARG((m + 31) / 32 <= 65535, "rart_gemm_small_m_bf16: m must stay below 2^21 rows (this is the small-M kernel)");
  hipLaunchKernelGGL(k_gemm_small_m, dim3((n + 31) / 32, (m + 31) / 32), dim3(kBlock), 0, (hipStream_t)stream, (const uint16_t*)a, lda,
                     (const uint16_t*)w, ldw, bias, out, ldo, out_is_f32, m, n, k);
  RART_CHECK_LAUNCH("rart_gemm_small_m_bf16");
  return RART_OK;
}

}  // extern "C"
