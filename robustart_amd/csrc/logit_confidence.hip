// Prediction, confidence and correctness over a class subset of fp32 logits for gfx950 (robustart_amd/metrics/confidence.py): what the
// ImageNet-A / ImageNet-O evaluation keeps of a sample, three numbers instead of the score vector.
//   z       = the K selected logits of a row in subset order (all `classes` of them without a subset)
//   pred    = the lowest position in [0, K) that attains max z (a NaN counts as larger than every number: numpy.argmax)
//   conf    = 1 / sum_j expf(z_j - z_pred): the largest soft-max probability over the subset, accurate expf, correctly rounded division
//   correct = pred == label (labels in subset coordinates; no labels: 0)
// One wave per row, rows grid-strided.  Lane l owns positions l, l + 64, l + 128, ...; it walks them in ascending order, so a strict
// "better than" keeps the lowest position of its maximum, and the cross-lane butterfly breaks ties towards the lower position.  The sum runs
// over four per-lane accumulators (position / 64 mod 4) in a fixed order, then the same butterfly: a row's outputs depend on its K values
// alone, never on the launch.  The special values need no branch: -inf - m is -inf (a term of 0) for a finite m, inf - inf and
// -inf - -inf are NaN, and a NaN maximum makes every term NaN.
//   K <= 1024: the row is read once into 16 registers per lane (positions past K read as -inf: they add 0 and lose every tie)
//   K  > 1024: two passes over the row, the second served by the cache (a 21 841-class row is 87 KB)
#include <math.h>

#include "rart_common.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRegVals = 16;               // values per lane of the register path
constexpr int kRegMaxK = 64 * kRegVals;

struct Best {
  float v;
  int j;
};

// does a value beat the lane's running best?  strict, so that the earlier position stays
__device__ __forceinline__ bool lc_beats(float v, float best) { return (v != v && best == best) || v > best; }

__device__ __forceinline__ Best lc_wave_best(Best b) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(b.v, off, 64);
    const int oj = __shfl_xor(b.j, off, 64);
    const bool same = ov == b.v || (ov != ov && b.v != b.v);
    if (lc_beats(ov, b.v) || (same && oj < b.j)) {
      b.v = ov;
      b.j = oj;
    }
  }
  return b;
}

__device__ __forceinline__ void lc_finish(int pred_j, const float acc[4], const int64_t* __restrict__ labels, int64_t r, int lane,
                                          int32_t* __restrict__ pred, float* __restrict__ conf, uint8_t* __restrict__ correct) {
  const float s = rart_wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if (lane == 0) {
    pred[r] = pred_j;
    conf[r] = 1.0f / s;
    correct[r] = labels != nullptr && labels[r] == (int64_t)pred_j ? 1 : 0;
  }
}

template <bool SUB>
__global__ __launch_bounds__(kBlock) void k_logit_conf_reg(const float* __restrict__ logits, int64_t rows, int64_t ld,
                                                           const int32_t* __restrict__ subset, int K, const int64_t* __restrict__ labels,
                                                           int32_t* __restrict__ pred, float* __restrict__ conf,
                                                           uint8_t* __restrict__ correct) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * kWaves;
  int col[kRegVals];                       // the same columns for every row of this wave
#pragma unroll
  for (int i = 0; i < kRegVals; ++i) {
    const int j = lane + 64 * i;
    col[i] = j < K ? (SUB ? subset[j] : j) : -1;
  }
  for (int64_t r = wave; r < rows; r += n_waves) {
    const float* __restrict__ row = logits + r * ld;
    float z[kRegVals];
#pragma unroll
    for (int i = 0; i < kRegVals; ++i) z[i] = col[i] >= 0 ? row[col[i]] : -INFINITY;
    Best b{z[0], lane};
#pragma unroll
    for (int i = 1; i < kRegVals; ++i)
      if (64 * i < K && lc_beats(z[i], b.v)) {          // (64 * i < K is the same for the whole wave: steps past K are skipped)
        b.v = z[i];
        b.j = lane + 64 * i;
      }
    b = lc_wave_best(b);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < kRegVals; ++i)
      if (64 * i < K) acc[i & 3] += expf(z[i] - b.v);
    lc_finish(b.j, acc, labels, r, lane, pred, conf, correct);
  }
}

template <bool SUB>
__global__ __launch_bounds__(kBlock) void k_logit_conf_loop(const float* __restrict__ logits, int64_t rows, int64_t ld,
                                                            const int32_t* __restrict__ subset, int K, const int64_t* __restrict__ labels,
                                                            int32_t* __restrict__ pred, float* __restrict__ conf,
                                                            uint8_t* __restrict__ correct) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * kWaves;
  const int steps = (K + 63) / 64, steps4 = (steps + 3) & ~3;        // whole groups of four: the accumulator of a step is a constant
  for (int64_t r = wave; r < rows; r += n_waves) {
    const float* __restrict__ row = logits + r * ld;
    auto at = [&](int i) -> float {
      const int j = lane + 64 * i;
      return j < K ? row[SUB ? subset[j] : j] : -INFINITY;
    };
    Best b{at(0), lane};
    for (int i = 1; i < steps; ++i) {
      const float v = at(i);
      if (lc_beats(v, b.v)) {
        b.v = v;
        b.j = lane + 64 * i;
      }
    }
    b = lc_wave_best(b);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < steps4; i += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] += expf(at(i + u) - b.v);
    }
    lc_finish(b.j, acc, labels, r, lane, pred, conf, correct);
  }
}
}  // namespace

extern "C" int rart_logit_confidence_f32(const float* logits, int64_t rows, int classes, int64_t ld, const int32_t* subset, int n_subset,
                                         const int64_t* labels, int32_t* pred, float* conf, uint8_t* correct, rart_stream_t stream) {
  RART_CHECK_ARG(rows >= 0, "rart_logit_confidence_f32: rows must not be negative, got %lld", (long long)rows);
  RART_CHECK_ARG(classes >= 1, "rart_logit_confidence_f32: classes must be at least 1, got %d", classes);
  RART_CHECK_ARG(ld >= classes, "rart_logit_confidence_f32: the row stride %lld is shorter than the %d classes", (long long)ld, classes);
  RART_CHECK_ARG(n_subset >= 0 && n_subset <= classes, "rart_logit_confidence_f32: a subset of %d of %d classes", n_subset, classes);
  if (rows == 0) return RART_OK;
  RART_CHECK_ARG(logits && pred && conf && correct, "rart_logit_confidence_f32: null pointer (logits, pred, conf and correct are required)");
  const bool sub = subset != nullptr && n_subset > 0;
  const int K = sub ? n_subset : classes;
  const int64_t blocks = (rows + kWaves - 1) / kWaves;
  const dim3 grid((unsigned)(blocks < 256 * 8 ? blocks : 256 * 8)), block(kBlock);
  hipStream_t st = (hipStream_t)stream;
  if (K <= kRegMaxK) {
    if (sub)
      hipLaunchKernelGGL(k_logit_conf_reg<true>, grid, block, 0, st, logits, rows, ld, subset, K, labels, pred, conf, correct);
    else
      hipLaunchKernelGGL(k_logit_conf_reg<false>, grid, block, 0, st, logits, rows, ld, subset, K, labels, pred, conf, correct);
  } else {
    if (sub)
      hipLaunchKernelGGL(k_logit_conf_loop<true>, grid, block, 0, st, logits, rows, ld, subset, K, labels, pred, conf, correct);
    else
      hipLaunchKernelGGL(k_logit_conf_loop<false>, grid, block, 0, st, logits, rows, ld, subset, K, labels, pred, conf, correct);
  }
  RART_CHECK_LAUNCH("rart_logit_confidence_f32");
  return RART_OK;
}
