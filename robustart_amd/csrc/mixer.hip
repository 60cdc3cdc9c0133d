// Token-mixing GEMM of MLP-Mixer (gfx950), in bf16 and in pair form:
//
//   C_b[m][n] = sum_k A[m][k] X_b[k][n]       per image b,  A = [M][lda] weights (K contiguous, shared by every image),
//                                                           X_b = [K][ldx] activations (n contiguous), C_b = [M][ldc]
//
// The contraction runs over the TOKEN axis of a [token][channel] activation, so the MFMA B operand (8 consecutive k of one column n)
// is k-strided in memory.  X tiles go global -> LDS as they are ([32 k][128 n], 256-byte rows, global_load_lds_dwordx4, 16-byte
// chunk c of row r stored at chunk c ^ 4 (r & 3)), and the fragments come out of LDS transposed with ds_read_b64_tr_b16, the
// wgrad_direct.hip recipe: a 16-lane group reads a [4 k][16 n] block and lane l receives column l of the four rows.  A tiles are
// [128 m][32 k] (64-byte rows, chunk c of row r at chunk c ^ ((r >> 2) & 3): the 16 rows a ds_read_b128 group reads fill one 256-byte
// bank window) and are read row-wise.  One activation is never transposed in HBM.
//
// Padding: X rows k >= K of an image are loaded from a zero line, never from the next image or past the allocation; A columns from K
// to the 32-multiple are zero in the table.  Output rows m >= M and columns n >= N are not stored.  No launch geometry or summation
// order depends on the batch, so an image's result is the same bits in any batch.  EXEC is all ones at every transposed read: the
// K loop is uniform and out-of-range pieces are padded from the zero line, not masked.
//
// Tile 128 x 128, four wave64s as 2 x 2 of 64 x 64 (2 x 2 v_mfma_f32_32x32x16_bf16 each), two-stage pipeline over 32-deep K steps.
// Pair form: hi and lo planes of both operands, three products hi.hi + hi.lo + lo.hi into one fp32 accumulator per K step (the
// arithmetic of rart_gemm_pair_bf16), hi / lo outputs.  Epilogue (fp32): + bias[m], + residual (may alias dst), then GELU (of the
// value rounded to the stored u, so a forward-only run and the kept forward agree), GELU with u kept in aux, or x GELU'(aux);
// bf16 / pair or fp32 output.
#include "rart_common.h"
#include "rart_bf16_helpers.h"
#include "rart_gemm_pair_dev.h"   // gp_gelu, gp_gelu_grad

namespace {
using namespace rart_bf16;
typedef __attribute__((ext_vector_type(4))) short tm_s16x4;
typedef __attribute__((ext_vector_type(8))) short tm_s16x8;

enum { TM_OUT_F32 = 2, TM_GELU = 4, TM_GELU_BWD = 8, TM_GELU_KEEP = 64 };
constexpr int TM_TM = 128, TM_TN = 128, TM_BK = 32;
constexpr int TM_A_BYTES = TM_TM * TM_BK * 2;       // 8 KiB: [128 m][32 k]
constexpr int TM_X_BYTES = TM_BK * TM_TN * 2;       // 8 KiB: [32 k][128 n]

struct TokmixDev {
  const uint16_t *a_hi, *a_lo, *x_hi, *x_lo;
  uint16_t *dst_hi, *dst_lo;
  const uint16_t *res_hi, *res_lo;
  uint16_t *aux_hi, *aux_lo;
  const float* bias;
  int M, N, K, lda, ldx, ldc, flags, k_steps;
  long long x_stride, c_stride;
};
__device__ __attribute__((aligned(16))) const uint32_t g_tm_zero16[4] = {0u, 0u, 0u, 0u};

// B fragment: 8 consecutive k (k0 .. k0 + 7) of column col0 + (lane & 15) of a [32][256-byte] X tile
__device__ __forceinline__ bf16x8 tm_x_frag(const uint8_t* tile, int k0, int col0, int a) {
  tm_s16x4 v[2];
#pragma unroll
  for (int rd = 0; rd < 2; ++rd) {
    const int row = k0 + 4 * rd + (a >> 2);
    const int colb = (col0 + 4 * (a & 3)) * 2;
    const int phys = (((colb >> 4) ^ (4 * (row & 3))) << 4) + (colb & 15);
    v[rd] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tm_s16x4*)(tile + row * 256 + phys));
  }
  const tm_s16x8 r = {v[0][0], v[0][1], v[0][2], v[0][3], v[1][0], v[1][1], v[1][2], v[1][3]};
  return __builtin_bit_cast(bf16x8, r);
}
// A fragment: row `row` of a [128][64-byte] A tile, logical 16-byte chunk c (k = 8c .. 8c + 7)
__device__ __forceinline__ bf16x8 tm_a_frag(const uint8_t* tile, int row, int c) {
  return *reinterpret_cast<const bf16x8*>(tile + row * 64 + 16 * (c ^ ((row >> 2) & 3)));
}
__device__ __forceinline__ uint16_t tm_rne(float v) {           // round to nearest even, the hardware conversion of pack_bf16x2
  return (uint16_t)(pack_bf16x2(v, 0.f) & 0xFFFFu);
}

template <bool PAIR>
__global__ __launch_bounds__(256) void k_tokmix(const TokmixDev d) {
  constexpr int NP = PAIR ? 2 : 1;
  constexpr int STAGE = NP * (TM_A_BYTES + TM_X_BYTES);
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
  const int n0 = blockIdx.x * TM_TN, m0 = blockIdx.y * TM_TM, b = blockIdx.z;
  const long long xoff = (long long)b * d.x_stride;
  // loader: wave w brings 1 KiB pieces 2w, 2w + 1 of the A tile (16 rows each) and of the X tile (4 rows each), per plane
  int a_row[2], a_chunk[2], x_row[2], x_col[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    a_row[q] = 16 * (2 * wave + q) + (lane >> 2);
    a_chunk[q] = (lane & 3) ^ ((a_row[q] >> 2) & 3);
    x_row[q] = 4 * (2 * wave + q) + (lane >> 4);
    x_col[q] = n0 + 8 * ((lane & 15) ^ (4 * (x_row[q] & 3)));
  }
  const char* const zsrc = reinterpret_cast<const char*>(g_tm_zero16);
#define RART_TM_DL(SRC, DST)                                                                                    \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(SRC),                        \
                                   (__attribute__((address_space(3))) void*)(DST), 16, 0, 0);
#define RART_TM_ISSUE(STEP, BUF)                                                                                \
  {                                                                                                             \
    uint8_t* const st_ = lds + (BUF)*STAGE;                                                                     \
    const int k0_ = (STEP)*TM_BK;                                                                               \
    _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                             \
      const bool ok_ = m0 + a_row[q] < d.M;                                                                     \
      const long long e_ = (long long)(m0 + a_row[q]) * d.lda + k0_ + 8 * a_chunk[q];                          \
      _Pragma("unroll") for (int p = 0; p < NP; ++p) {                                                          \
        const uint16_t* const pl_ = p ? d.a_lo : d.a_hi;                                                        \
        RART_TM_DL(ok_ ? reinterpret_cast<const char*>(pl_ + e_) : zsrc, st_ + p * TM_A_BYTES + (2 * wave + q) * 1024) \
      }                                                                                                         \
    }                                                                                                           \
    _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                             \
      const bool ok_ = k0_ + x_row[q] < d.K && x_col[q] < d.N;                                                  \
      const long long e_ = xoff + (long long)(k0_ + x_row[q]) * d.ldx + x_col[q];                               \
      _Pragma("unroll") for (int p = 0; p < NP; ++p) {                                                          \
        const uint16_t* const pl_ = p ? d.x_lo : d.x_hi;                                                        \
        RART_TM_DL(ok_ ? reinterpret_cast<const char*>(pl_ + e_) : zsrc,                                        \
                   st_ + NP * TM_A_BYTES + p * TM_X_BYTES + (2 * wave + q) * 1024)                               \
      }                                                                                                         \
    }                                                                                                           \
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int g = lane >> 4, a = lane & 15, h = lane >> 5, fr = lane & 31;
  RART_TM_ISSUE(0, 0)
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  for (int s = 0; s < d.k_steps; ++s) {
    const int buf = s & 1;
    if (s + 1 < d.k_steps) RART_TM_ISSUE(s + 1, buf ^ 1)
    const uint8_t* const At = lds + buf * STAGE;
    const uint8_t* const Xt = At + NP * TM_A_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int k0 = ks * 16 + 8 * (g >> 1);
      bf16x8 af[NP][2], xf[NP][2];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int i = 0; i < 2; ++i) af[p][i] = tm_a_frag(At + p * TM_A_BYTES, wm * 64 + i * 32 + fr, 2 * ks + h);
#pragma unroll
        for (int j = 0; j < 2; ++j) xf[p][j] = tm_x_frag(Xt + p * TM_X_BYTES, k0, wn * 64 + j * 32 + 16 * (g & 1), a);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], xf[0][j], acc[i][j], 0, 0, 0);
          if (PAIR) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][i], xf[NP - 1][j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[NP - 1][i], xf[0][j], acc[i][j], 0, 0, 0);
          }
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }
#undef RART_TM_ISSUE
#undef RART_TM_DL
  // ---- epilogue: acc[i][j][r] = row wm*64 + i*32 + (r&3) + 8*(r>>2) + 4h, column wn*64 + j*32 + (lane & 31); a wave store covers
  //      32 consecutive columns of one row
  const long long coff = (long long)b * d.c_stride;
  const int flags = d.flags;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn * 64 + j * 32 + fr;
      if (col >= d.N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row >= d.M) continue;
        const long long e = coff + (long long)row * d.ldc + col;
        float v = acc[i][j][r];
        if (d.bias) v += d.bias[row];
        if (d.res_hi) v += PAIR ? bf2f(d.res_hi[e]) + bf2f(d.res_lo[e]) : bf2f(d.res_hi[e]);
        if (flags & (TM_GELU | TM_GELU_KEEP)) {
          const uint16_t uh = tm_rne(v);
          const uint16_t ul = PAIR ? tm_rne(v - bf2f(uh)) : 0;
          if (flags & TM_GELU_KEEP) {
            d.aux_hi[e] = uh;
            if (PAIR) d.aux_lo[e] = ul;
          }
          v = gp_gelu(PAIR ? bf2f(uh) + bf2f(ul) : bf2f(uh));
        }
        if (flags & TM_GELU_BWD) v *= gp_gelu_grad(PAIR ? bf2f(d.aux_hi[e]) + bf2f(d.aux_lo[e]) : bf2f(d.aux_hi[e]));
        if (flags & TM_OUT_F32) {
          reinterpret_cast<float*>(d.dst_hi)[e] = v;
        } else {
          const uint16_t oh = tm_rne(v);
          d.dst_hi[e] = oh;
          if (PAIR) d.dst_lo[e] = tm_rne(v - bf2f(oh));
        }
      }
    }
}

bool tm_aligned(const void* p) { return p == nullptr || ((uintptr_t)p & 15u) == 0; }

int tokmix_launch(const rart_tokmix_desc* h, bool pair, rart_stream_t stream, const char* what) {
  RART_CHECK_ARG(h != nullptr, "%s: null descriptor", what);
  RART_CHECK_ARG(h->a_hi && h->x_hi && h->dst_hi && (!pair || (h->a_lo && h->x_lo)), "%s: null operand", what);
  RART_CHECK_ARG(h->M > 0 && h->N > 0 && h->K > 0 && h->batch > 0 && h->batch <= 65535, "%s: bad sizes (M %d, N %d, K %d, batch %d)", what,
                 h->M, h->N, h->K, h->batch);
  const int k_pad = (h->K + TM_BK - 1) / TM_BK * TM_BK;
  RART_CHECK_ARG(h->lda >= k_pad && h->lda % 8 == 0, "%s: lda %d must be a multiple of 8 and cover K rounded up to 32 (%d)", what, h->lda, k_pad);
  RART_CHECK_ARG(h->N % 8 == 0 && h->ldx >= h->N && h->ldx % 8 == 0 && h->ldc >= h->N && h->x_stride % 8 == 0,
                 "%s: N, ldx and x_stride must be multiples of 8, ldx and ldc >= N", what);
  RART_CHECK_ARG(h->x_stride >= (long long)h->K * h->ldx && h->c_stride >= (long long)h->M * h->ldc,
                 "%s: an image's slab must hold K (M) rows: x_stride >= K ldx, c_stride >= M ldc", what);
  RART_CHECK_ARG(tm_aligned(h->a_hi) && tm_aligned(h->a_lo) && tm_aligned(h->x_hi) && tm_aligned(h->x_lo),
                 "%s: A and X planes must be 16-byte aligned", what);
  const int f = h->flags;
  RART_CHECK_ARG((f & ~(TM_OUT_F32 | TM_GELU | TM_GELU_BWD | TM_GELU_KEEP)) == 0, "%s: unknown flags %d", what, f);
  RART_CHECK_ARG(__builtin_popcount(f & (TM_GELU | TM_GELU_BWD | TM_GELU_KEEP)) <= 1, "%s: at most one GELU form", what);
  RART_CHECK_ARG(!(f & (TM_GELU_BWD | TM_GELU_KEEP)) || (h->aux_hi && (!pair || h->aux_lo)), "%s: flags 8 / 64 need aux", what);
  RART_CHECK_ARG(!((f & TM_OUT_F32) && (f & TM_GELU_KEEP)), "%s: flag 64 writes bf16 outputs", what);
  RART_CHECK_ARG((f & TM_OUT_F32) || !pair || h->dst_lo, "%s: the pair form needs dst_lo", what);
  RART_CHECK_ARG(!pair || !h->res_hi || h->res_lo, "%s: the pair form needs res_lo with res_hi", what);
  RART_CHECK_ARG((long long)(h->M + TM_TM) * h->lda < (1ll << 31), "%s: the weight table must stay below 2^31 elements", what);
  TokmixDev d;
  d.a_hi = (const uint16_t*)h->a_hi; d.a_lo = (const uint16_t*)h->a_lo;
  d.x_hi = (const uint16_t*)h->x_hi; d.x_lo = (const uint16_t*)h->x_lo;
  d.dst_hi = (uint16_t*)h->dst_hi; d.dst_lo = (uint16_t*)h->dst_lo;
  d.res_hi = (const uint16_t*)h->res_hi; d.res_lo = (const uint16_t*)h->res_lo;
  d.aux_hi = (uint16_t*)h->aux_hi; d.aux_lo = (uint16_t*)h->aux_lo;
  d.bias = h->bias;
  d.M = h->M; d.N = h->N; d.K = h->K; d.lda = h->lda; d.ldx = h->ldx; d.ldc = h->ldc; d.flags = f;
  d.k_steps = k_pad / TM_BK;
  d.x_stride = h->x_stride; d.c_stride = h->c_stride;
  const dim3 grid((h->N + TM_TN - 1) / TM_TN, (h->M + TM_TM - 1) / TM_TM, h->batch);
  if (pair) hipLaunchKernelGGL(k_tokmix<true>, grid, dim3(256), 0, (hipStream_t)stream, d);
  else hipLaunchKernelGGL(k_tokmix<false>, grid, dim3(256), 0, (hipStream_t)stream, d);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}
}  // namespace

extern "C" int rart_tokmix_bf16(const rart_tokmix_desc* desc, rart_stream_t stream) {
  return tokmix_launch(desc, false, stream, "rart_tokmix_bf16");
}

extern "C" int rart_tokmix_pair(const rart_tokmix_desc* desc, rart_stream_t stream) {
  return tokmix_launch(desc, true, stream, "rart_tokmix_pair");
}
