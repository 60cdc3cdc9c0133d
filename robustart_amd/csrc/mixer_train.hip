// Gradients of MLP-Mixer's token-mixing parameters (gfx950, bf16 training):
//
//   G[m][n] = sum_b sum_d P_b[m][d] Q_b[n][d]       P = [batch][M][D], Q = [batch][N][D] per-image slabs, D contiguous
//   s[m]    = sum_b sum_d X_b[m][d]                 the token biases
//
// dW1[h][t] is this product with P = d(u_tok) and Q = LN1(x), dW2[t][h] with P = dx' and Q = gelu(u_tok).  Both operands are contiguous
// along the contraction axis, so both tiles are [128 rows][32 d] with 64-byte rows (k_tokmix's A tile: 16-byte LDS-DMA loads, chunk c of
// row r at chunk c ^ ((r >> 2) & 3), fragments by ds_read_b128) and nothing is read transposed or copied transposed in HBM.  The
// contraction is batch x D long and the output tiny, so blockIdx.z splits it over images: split z walks images
// [z * images_per_split, (z + 1) * images_per_split) in order and writes the fp32 tile C[n][m] to partial[z][n][m] (row stride
// ld_partial), the [splits][in][out] layout rart_wgrad_reduce_f32 folds with taps = 1 into torch's [out][in] gradient.  No atomics:
// every sum has a fixed order, two runs give the same bits.
//
// Padding: rows m >= M / n >= N and 16-byte chunks at d >= D are loaded from a zero line, never from the next slab or past the
// allocation; D is a multiple of 8, so a chunk is inside a row or outside it.  A split with no image writes zeros.
//
// Tile 128 (n) x 128 (m), four wave64s as 2 x 2 of 64 x 64 (2 x 2 v_mfma_f32_32x32x16_bf16 each), two-stage pipeline over 32-deep steps.
// The MFMA row operand is Q and the column operand P, so an accumulator's lanes run along m and a wave store covers 32 consecutive
// floats of one partial row.
#include "rart_common.h"
#include "rart_bf16_helpers.h"

namespace {
constexpr int TW_T = 128, TW_BK = 32;
constexpr int TW_TILE_BYTES = TW_T * TW_BK * 2;       // 8 KiB: [128 rows][32 d]
constexpr int TW_STAGE = 2 * TW_TILE_BYTES;           // Q tile, P tile
constexpr int TW_ROWSUM_CHUNKS = 32;

struct TokWgradDev {
  const uint16_t *p, *q;
  float* partial;
  int M, N, D, batch, ips, ldp, d_pad;
  long long p_stride, q_stride;
};
__device__ __attribute__((aligned(16))) const uint32_t g_tw_zero16[4] = {0u, 0u, 0u, 0u};

// fragment: row `row` of a [128][64-byte] tile, logical 16-byte chunk c (d = 8c .. 8c + 7)
__device__ __forceinline__ bf16x8 tw_frag(const uint8_t* tile, int row, int c) {
  return *reinterpret_cast<const bf16x8*>(tile + row * 64 + 16 * (c ^ ((row >> 2) & 3)));
}

__global__ __launch_bounds__(256) void k_tokmix_wgrad(const TokWgradDev d) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * TW_STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * TW_T, n0 = blockIdx.y * TW_T, z = blockIdx.z;
  const int b0 = z * d.ips, b1 = b0 + d.ips < d.batch ? b0 + d.ips : d.batch;
  const int steps = b1 > b0 ? (b1 - b0) * (d.d_pad / TW_BK) : 0;
  // loader: wave w brings 1 KiB pieces 2w, 2w + 1 (16 rows each) of the Q tile and of the P tile
  int row[2], chunk[2];
  long long q_off[2], p_off[2];
  bool q_ok[2], p_ok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    row[i] = 16 * (2 * wave + i) + (lane >> 2);
    chunk[i] = (lane & 3) ^ ((row[i] >> 2) & 3);
    q_ok[i] = n0 + row[i] < d.N;
    p_ok[i] = m0 + row[i] < d.M;
    q_off[i] = (long long)(n0 + row[i]) * d.D + 8 * chunk[i];
    p_off[i] = (long long)(m0 + row[i]) * d.D + 8 * chunk[i];
  }
  const char* const zsrc = reinterpret_cast<const char*>(g_tw_zero16);
#define RART_TW_DL(SRC, DST)                                                                                    \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(SRC),                        \
                                   (__attribute__((address_space(3))) void*)(DST), 16, 0, 0);
  // the step to load next: image ld_b, channel offset ld_k (wave-uniform)
  int ld_b = b0, ld_k = 0;
#define RART_TW_ISSUE(BUF)                                                                                      \
  {                                                                                                             \
    uint8_t* const st_ = lds + (BUF)*TW_STAGE;                                                                  \
    const uint16_t* const qb_ = d.q + (long long)ld_b * d.q_stride + ld_k;                                      \
    const uint16_t* const pb_ = d.p + (long long)ld_b * d.p_stride + ld_k;                                      \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                             \
      const bool in_ = ld_k + 8 * chunk[i] < d.D;                                                               \
      RART_TW_DL(q_ok[i] && in_ ? reinterpret_cast<const char*>(qb_ + q_off[i]) : zsrc, st_ + (2 * wave + i) * 1024) \
      RART_TW_DL(p_ok[i] && in_ ? reinterpret_cast<const char*>(pb_ + p_off[i]) : zsrc,                         \
                 st_ + TW_TILE_BYTES + (2 * wave + i) * 1024)                                                    \
    }                                                                                                           \
    ld_k += TW_BK;                                                                                              \
    if (ld_k >= d.d_pad) { ld_k = 0; ++ld_b; }                                                                  \
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int h = lane >> 5, fr = lane & 31;
  if (steps > 0) {
    RART_TW_ISSUE(0)
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    if (s + 1 < steps) RART_TW_ISSUE(buf ^ 1)
    const uint8_t* const Qt = lds + buf * TW_STAGE;
    const uint8_t* const Pt = Qt + TW_TILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 qf[2], pf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) qf[i] = tw_frag(Qt, wm * 64 + i * 32 + fr, 2 * ks + h);
#pragma unroll
      for (int j = 0; j < 2; ++j) pf[j] = tw_frag(Pt, wn * 64 + j * 32 + fr, 2 * ks + h);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[i], pf[j], acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }
#undef RART_TW_ISSUE
#undef RART_TW_DL
  // acc[i][j][r] = C[n = wm*64 + i*32 + (r&3) + 8*(r>>2) + 4h][m = wn*64 + j*32 + (lane & 31)]
  float* const out = d.partial + (long long)z * d.N * d.ldp;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = m0 + wn * 64 + j * 32 + fr;
      if (m >= d.M) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (n < d.N) out[(long long)n * d.ldp + m] = acc[i][j][r];
      }
    }
}

__device__ __forceinline__ float tw_sum8(const uint4& v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) a += __uint_as_float(w[j] << 16) + __uint_as_float(w[j] & 0xFFFF0000u);
  return a;
}

// partial[c][m] = sum over the images of chunk c and the channels of x[b][m][:]: one workgroup per (row, chunk)
__global__ __launch_bounds__(256) void k_tok_rowsum(const uint16_t* __restrict__ x, int rows, int dim, int batch, int ipc,
                                                    long long stride, float* __restrict__ partial) {
  __shared__ float ws[4];
  const int m = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int b0 = c * ipc, b1 = b0 + ipc < batch ? b0 + ipc : batch;
  const int v = dim / 8, total = b1 > b0 ? (b1 - b0) * v : 0;
  float a = 0.f;
  for (int i = tid; i < total; i += 256) {
    const int ib = i / v, iv = i - ib * v;
    a += tw_sum8(*reinterpret_cast<const uint4*>(x + (long long)(b0 + ib) * stride + (long long)m * dim + 8 * iv));
  }
  a = rart_wave_sum(a);
  if ((tid & 63) == 0) ws[tid >> 6] = a;
  __syncthreads();
  if (tid == 0) partial[(size_t)c * rows + m] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

__global__ __launch_bounds__(256) void k_tok_rowsum_fold(const float* __restrict__ partial, int chunks, int rows, float* __restrict__ out,
                                                         int accumulate) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= rows) return;
  float a = 0.f;
  for (int c = 0; c < chunks; ++c) a += partial[(size_t)c * rows + m];      // fixed order
  out[m] = accumulate ? out[m] + a : a;
}

bool tw_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }
int tw_rowsum_chunks(int batch) {
  const int ipc = (batch + TW_ROWSUM_CHUNKS - 1) / TW_ROWSUM_CHUNKS;
  return (batch + ipc - 1) / ipc;
}
}  // namespace

extern "C" int rart_tokmix_wgrad_bf16(const rart_tokmix_wgrad_desc* h, rart_stream_t stream) {
  const char* const what = "rart_tokmix_wgrad_bf16";
  RART_CHECK_ARG(h != nullptr, "%s: null descriptor", what);
  RART_CHECK_ARG(h->p && h->q && h->partial, "%s: null operand", what);
  RART_CHECK_ARG(h->M > 0 && h->N > 0 && h->D > 0 && h->batch > 0 && h->splits > 0 && h->splits <= 65535 && h->images_per_split > 0,
                 "%s: bad sizes (M %d, N %d, D %d, batch %d, splits %d, images_per_split %d)", what, h->M, h->N, h->D, h->batch, h->splits,
                 h->images_per_split);
  RART_CHECK_ARG(h->D % 8 == 0, "%s: D %d must be a multiple of 8", what, h->D);
  RART_CHECK_ARG(h->p_stride % 8 == 0 && h->q_stride % 8 == 0 && h->p_stride >= (long long)h->M * h->D &&
                     h->q_stride >= (long long)h->N * h->D,
                 "%s: an image's slab must hold its rows: p_stride >= M D, q_stride >= N D, multiples of 8", what);
  RART_CHECK_ARG(tw_aligned(h->p) && tw_aligned(h->q), "%s: P and Q planes must be 16-byte aligned", what);
  RART_CHECK_ARG(((uintptr_t)h->partial & 3u) == 0 && h->ld_partial >= h->M, "%s: ld_partial %d must cover M %d (fp32 partial)", what,
                 h->ld_partial, h->M);
  RART_CHECK_ARG((long long)h->splits * h->images_per_split >= h->batch,
                 "%s: splits * images_per_split (%d x %d) must cover the batch %d", what, h->splits, h->images_per_split, h->batch);
  TokWgradDev d;
  d.p = (const uint16_t*)h->p; d.q = (const uint16_t*)h->q; d.partial = h->partial;
  d.M = h->M; d.N = h->N; d.D = h->D; d.batch = h->batch; d.ips = h->images_per_split; d.ldp = h->ld_partial;
  d.d_pad = (h->D + TW_BK - 1) / TW_BK * TW_BK;
  d.p_stride = h->p_stride; d.q_stride = h->q_stride;
  const dim3 grid((h->M + TW_T - 1) / TW_T, (h->N + TW_T - 1) / TW_T, h->splits);
  hipLaunchKernelGGL(k_tokmix_wgrad, grid, dim3(256), 0, (hipStream_t)stream, d);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}

extern "C" size_t rart_tok_rowsum_workspace_bytes(int rows, int batch) {
  if (rows <= 0 || batch <= 0) return 0;
  return (size_t)tw_rowsum_chunks(batch) * rows * sizeof(float);
}

extern "C" int rart_tok_rowsum_bf16(const void* x, int rows, int dim, int batch, int64_t stride, float* out, int accumulate,
                                    void* workspace, size_t workspace_bytes, rart_stream_t stream) {
  const char* const what = "rart_tok_rowsum_bf16";
  RART_CHECK_ARG(x && out, "%s: null operand", what);
  RART_CHECK_ARG(rows > 0 && rows <= 65535 && dim > 0 && batch > 0, "%s: bad sizes (rows %d, dim %d, batch %d)", what, rows, dim, batch);
  RART_CHECK_ARG(dim % 8 == 0, "%s: dim %d must be a multiple of 8", what, dim);
  RART_CHECK_ARG(stride % 8 == 0 && stride >= (long long)rows * dim, "%s: an image's slab must hold its rows: stride >= rows dim, a multiple of 8",
                 what);
  RART_CHECK_ARG(tw_aligned(x), "%s: x must be 16-byte aligned", what);
  const size_t need = rart_tok_rowsum_workspace_bytes(rows, batch);
  if (!workspace || workspace_bytes < need) {
    rart_set_error("%s: workspace of %zu bytes required", what, need);
    return RART_ERR_WORKSPACE;
  }
  const int chunks = tw_rowsum_chunks(batch), ipc = (batch + TW_ROWSUM_CHUNKS - 1) / TW_ROWSUM_CHUNKS;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tok_rowsum, dim3(rows, chunks), dim3(256), 0, st, (const uint16_t*)x, rows, dim, batch, ipc, (long long)stride,
                     (float*)workspace);
  hipLaunchKernelGGL(k_tok_rowsum_fold, dim3((rows + 255) / 256), dim3(256), 0, st, (const float*)workspace, chunks, rows, out, accumulate);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}
