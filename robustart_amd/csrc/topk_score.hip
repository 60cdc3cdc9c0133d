// Prediction, label rank and top-k hit counters of fp32 logits for gfx950 (robustart_amd/metrics/confidence.py: topk_score): what the
// ImageNet-C loop keeps of a batch, 8 bytes per sample and two counters per (corruption, severity) instead of the score vectors.
//   z       = the first `classes` values of a row, y = labels[r]
//   rank    = #{j : z_j > z_y} + #{j < y : z_j == z_y}: the position of the label in a stable descending sort (ties to the lower class
//             index); `classes` for a label outside [0, classes) or a NaN z_y.  IEEE compares: a NaN elsewhere never outranks.
//   pred    = the lowest index that attains max z (a NaN counts as larger than every number: numpy.argmax)
//   hits[i] += #{r : rank[r] < ks[i] and rank[r] < classes} (a rank of `classes` is a miss for every k, also for a k above classes)
// One wave per row, rows grid-strided, four waves per workgroup.  Both outputs need one value besides the row itself (z_y, one
// broadcast load), so the row is read ONCE whatever its length: nothing is kept in registers and 21 841 classes take the same loop
// as 1000.  Lane l owns elements l, l + 64, ... (or quads 4l .. 4l + 3, 4(l + 64) .., when base and row stride allow 16-byte
// loads); it walks them in ascending order, so a strict "better than" keeps the lowest index of its maximum, and the cross-lane
// butterfly breaks ties towards the lower index.  The counts are integers: neither the element-to-lane mapping nor the order of the
// atomic adds can change a result, and a row's outputs depend on that row alone.
// Counters: every wave counts its rows' hits in registers (the rank is wave-uniform after the butterfly sum), the four waves meet
// in LDS, and one thread per k issues one 64-bit global_atomic_add per workgroup (none when the workgroup has no hit).
#include <limits.h>
#include <math.h>

#include "rart_common.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxBlocks = 256 * 8;        // rows per trip of the grid-stride loop: kMaxBlocks * kWaves = 8192
constexpr int kMaxK = 8;

struct Ks {
  int k[kMaxK];
};

struct Best {
  float v;
  int j;                                   // INT_MAX: nothing seen yet (loses every tie)
};

// does a value beat the running best?  strict, so that the earlier index stays
__device__ __forceinline__ bool ts_beats(float v, float best) { return (v != v && best == best) || v > best; }

__device__ __forceinline__ Best ts_wave_best(Best b) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(b.v, off, 64);
    const int oj = __shfl_xor(b.j, off, 64);
    const bool same = ov == b.v || (ov != ov && b.v != b.v);
    if (ts_beats(ov, b.v) || (same && oj < b.j)) {          // (a lane that saw nothing holds (-inf, INT_MAX): it wins no tie)
      b.v = ov;
      b.j = oj;
    }
  }
  return b;
}

__device__ __forceinline__ int ts_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_topk_score(const float* __restrict__ logits, int64_t rows, int classes, int64_t ld,
                                                       const int64_t* __restrict__ labels, int32_t* __restrict__ pred,
                                                       int32_t* __restrict__ rank, Ks ks, int n_k, unsigned long long* __restrict__ hits) {
  __shared__ unsigned long long s_cnt[kWaves][kMaxK];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t wave = (int64_t)blockIdx.x * kWaves + w, n_waves = (int64_t)gridDim.x * kWaves;
  unsigned long long cnt[kMaxK];
#pragma unroll
  for (int i = 0; i < kMaxK; ++i) cnt[i] = 0;
  for (int64_t r = wave; r < rows; r += n_waves) {
    const float* __restrict__ row = logits + r * ld;
    const int64_t y64 = labels[r];
    const bool valid = y64 >= 0 && y64 < (int64_t)classes;
    const int y = valid ? (int)y64 : 0;
    const float zy = valid ? row[y] : __builtin_nanf("");       // NaN: every compare below is false, the rank is overridden
    Best b{-INFINITY, INT_MAX};
    int above = 0;
    auto visit = [&](float v, int j) {
      above += (v > zy ? 1 : 0) + ((v == zy && j < y) ? 1 : 0);
      if (b.j == INT_MAX || ts_beats(v, b.v)) {
        b.v = v;
        b.j = j;
      }
    };
    if (VEC) {
      const int64_t nq = ((int64_t)classes + 3) >> 2;
#pragma unroll 2
      for (int64_t q = lane; q < nq; q += 64) {
        const int64_t j0 = q << 2;
        if (j0 + 3 < classes) {
          const float4 v = *reinterpret_cast<const float4*>(row + j0);
          visit(v.x, (int)j0);
          visit(v.y, (int)j0 + 1);
          visit(v.z, (int)j0 + 2);
          visit(v.w, (int)j0 + 3);
        } else {                                                  // the last quad of a row whose length is no multiple of 4
          for (int64_t j = j0; j < classes; ++j) visit(row[j], (int)j);
        }
      }
    } else {
#pragma unroll 4
      for (int64_t j = lane; j < classes; j += 64) visit(row[j], (int)j);
    }
    above = ts_wave_sum(above);
    b = ts_wave_best(b);
    const int rk = (!valid || zy != zy) ? classes : above;
    if (lane == 0) {
      if (pred != nullptr) pred[r] = b.j;
      if (rank != nullptr) rank[r] = rk;
    }
#pragma unroll
    for (int i = 0; i < kMaxK; ++i) cnt[i] += (i < n_k && rk < classes && rk < ks.k[i]) ? 1u : 0u;   // rank == classes misses every k
  }
  if (hits == nullptr) return;                                    // (uniform over the grid)
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kMaxK; ++i) s_cnt[w][i] = cnt[i];
  }
  __syncthreads();
  if ((int)threadIdx.x < n_k) {
    unsigned long long s = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) s += s_cnt[v][threadIdx.x];
    if (s != 0) atomicAdd(hits + threadIdx.x, s);
  }
}
}  // namespace

extern "C" int rart_topk_score_f32(const float* logits, int64_t rows, int classes, int64_t ld, const int64_t* labels, int32_t* pred,
                                   int32_t* rank, const int* ks, int n_k, int64_t* hits, rart_stream_t stream) {
  RART_CHECK_ARG(rows >= 0, "rart_topk_score_f32: rows must not be negative, got %lld", (long long)rows);
  RART_CHECK_ARG(classes >= 1, "rart_topk_score_f32: classes must be at least 1, got %d", classes);
  RART_CHECK_ARG(ld >= classes, "rart_topk_score_f32: the row stride %lld is shorter than the %d classes", (long long)ld, classes);
  RART_CHECK_ARG(n_k >= 0 && n_k <= kMaxK, "rart_topk_score_f32: n_k must lie in [0, %d], got %d", kMaxK, n_k);
  RART_CHECK_ARG(n_k == 0 || ks != nullptr, "rart_topk_score_f32: null ks with n_k = %d", n_k);
  Ks kk{};
  for (int i = 0; i < n_k; ++i) {
    RART_CHECK_ARG(ks[i] >= 1, "rart_topk_score_f32: ks[%d] must be at least 1, got %d", i, ks[i]);
    kk.k[i] = ks[i];
  }
  if (rows == 0) return RART_OK;
  RART_CHECK_ARG(logits && labels, "rart_topk_score_f32: null pointer (logits and labels are required)");
  if (hits == nullptr) n_k = 0;
  if (n_k == 0) hits = nullptr;
  const int64_t blocks = (rows + kWaves - 1) / kWaves;
  const dim3 grid((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), block(kBlock);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hits);
  // 16-byte loads need every row to start on a 16-byte boundary: the base does and the stride is a multiple of four floats
  const bool vec = ((uintptr_t)logits & 15u) == 0 && (ld & 3) == 0;
  if (vec)
    hipLaunchKernelGGL(k_topk_score<true>, grid, block, 0, st, logits, rows, classes, ld, labels, pred, rank, kk, n_k, h);
  else
    hipLaunchKernelGGL(k_topk_score<false>, grid, block, 0, st, logits, rows, classes, ld, labels, pred, rank, kk, n_k, h);
  RART_CHECK_LAUNCH("rart_topk_score_f32");
  return RART_OK;
}
