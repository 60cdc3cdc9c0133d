// torchvision's ColorJitter on a uint8 NHWC batch for gfx950, bit for bit what Pillow computes (robustart_amd/train/jitter.py).
// Per sample a record (rart_jitter_rec) names up to four operations in application order:
//   0 brightness  Image.blend(black, img, f)                       ImageEnhance.Brightness
//   1 contrast    Image.blend(grey(m), img, f), m = the rounded mean of L over the image AS IT IS when the slot is reached
//   2 saturation  Image.blend(L as RGB, img, f)                    ImageEnhance.Color
//   3 hue         RGB -> HSV, H += shift (mod 256), HSV -> RGB     Pillow's convert('HSV') / convert('RGB'); not the identity at shift 0
//   L     = (19595 R + 38470 G + 7471 B + 32768) >> 16                                            Pillow's convert('L')
//   blend = clamp to [0, 255] and truncate (float)a + alpha * ((float)b - (float)a), fp32, product and sum rounded separately
// Every operation but the contrast mean is a pure function of one pixel, so the entry is two launches:
//   1. samples with a contrast slot: the slots before it are recomputed per pixel, L is summed per wave, per workgroup, and added to
//      lsum[sample] with one integer atomic per workgroup (integer addition: the sum does not depend on the order);
//   2. all slots per pixel, m = (2 * lsum + count) / (2 * count), one write.
// Two reads and one write of the batch.  A thread owns four consecutive pixels of one image: three dwords in, three out, when the
// pointers and h * w allow it; the same arithmetic byte by byte otherwise.
#include "rart_common.h"

// plain operators under contract(off), as in batch_mix.hip: a fused multiply-add in the blend differs from Pillow on thousands of (a, b) pairs
#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr uint32_t kSkip = 4;

struct CjPlan {
  uint32_t op[4];        // sanitized: 0..3, or kSkip (an id outside 0..3, or one that an earlier slot already carries)
  float f[3];
  uint32_t shift;
  int contrast_slot;     // -1: none
};

__host__ __device__ inline CjPlan cj_decode(const rart_jitter_rec& r) {
  CjPlan p;
  uint32_t seen = 0;
  p.contrast_slot = -1;
  for (int k = 0; k < 4; ++k) {
    uint32_t id = r.op[k];
    if (id > 3u || ((seen >> id) & 1u)) id = kSkip;
    else seen |= 1u << id;
    if (id == 1u) p.contrast_slot = k;
    p.op[k] = id;
  }
  for (int k = 0; k < 3; ++k) p.f[k] = r.factor[k];
  p.shift = r.hue_shift & 255u;
  return p;
}

__host__ __device__ inline uint32_t cj_luma(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }

__host__ __device__ inline uint32_t cj_blend(uint32_t a, uint32_t b, float alpha) {
  const float fa = (float)a;
  const float d = (float)b - fa;
  const float p = alpha * d;
  const float s = fa + p;
  return !(s > 0.0f) ? 0u : (s >= 255.0f ? 255u : (uint32_t)s);
}

// Pillow's rgb2hsv_row, the hue shift, hsv2rgb_row.  x - floor(x) stands for fmod(x, 1.0): x = h / 6 + 1 lies in [5/6, 11/6], where both are exact.
__host__ __device__ inline void cj_hue(uint32_t shift, uint32_t& r, uint32_t& g, uint32_t& b) {
  const uint32_t maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const uint32_t minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  if (maxc == minc) return;                      // S = 0: grey V whatever H is, and r = g = b = V already
  const float cr = (float)(maxc - minc);
  const float s = cr / (float)maxc;
  const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
  float h;
  if (r == maxc) h = bc - gc;
  else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
  else h = (float)(4.0 + (double)gc - (double)rc);
  const double x = (double)h / 6.0 + 1.0;
  h = (float)(x - floor(x));
  int hi = (int)((double)h * 255.0), si = (int)((double)s * 255.0);
  hi = hi < 0 ? 0 : (hi > 255 ? 255 : hi);
  si = si < 0 ? 0 : (si > 255 ? 255 : si);
  const uint32_t H = ((uint32_t)hi + shift) & 255u, V = maxc;
  if (si == 0) {
    r = g = b = V;
    return;
  }
  const double hh = (double)H * 6.0 / 255.0;
  const double fl = floor(hh);
  const float f = (float)(hh - fl);
  const float fs = (float)((double)si / 255.0);
  const double v = (double)V, dfs = (double)fs, df = (double)f;
  const uint32_t p = (uint32_t)round(v * (1.0 - dfs));          // half away from zero; every argument is >= 0
  const uint32_t q = (uint32_t)round(v * (1.0 - dfs * df));
  const uint32_t t = (uint32_t)round(v * (1.0 - dfs * (1.0 - df)));
  switch ((int)fl % 6) {
    case 0: r = V, g = t, b = p; break;
    case 1: r = q, g = V, b = p; break;
    case 2: r = p, g = V, b = t; break;
    case 3: r = p, g = q, b = V; break;
    case 4: r = t, g = p, b = V; break;
    default: r = V, g = p, b = q; break;
  }
}

// slots [0, stop) of the plan on one pixel; `mean` is read by a contrast slot only
__host__ __device__ inline void cj_apply(const CjPlan& p, int stop, uint32_t mean, uint32_t& r, uint32_t& g, uint32_t& b) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {                   // unrolled: the plan stays in registers
    if (k >= stop) break;
    switch (p.op[k]) {
      case 0: r = cj_blend(0u, r, p.f[0]), g = cj_blend(0u, g, p.f[0]), b = cj_blend(0u, b, p.f[0]); break;
      case 1: r = cj_blend(mean, r, p.f[1]), g = cj_blend(mean, g, p.f[1]), b = cj_blend(mean, b, p.f[1]); break;
      case 2: {
        const uint32_t l = cj_luma(r, g, b);
        r = cj_blend(l, r, p.f[2]), g = cj_blend(l, g, p.f[2]), b = cj_blend(l, b, p.f[2]);
        break;
      }
      case 3: cj_hue(p.shift, r, g, b); break;
      default: break;
    }
  }
}

__device__ __forceinline__ void cj_load(const uint8_t* p, bool vec, uint32_t cnt, uint32_t v[12]) {
  if (vec) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    const uint32_t d[3] = {q[0], q[1], q[2]};
#pragma unroll
    for (int j = 0; j < 12; ++j) v[j] = (d[j / 4] >> (8 * (j % 4))) & 255u;
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j) v[j] = (uint32_t)j < cnt * 3u ? p[j] : 0u;
  }
}

__device__ __forceinline__ void cj_store(uint8_t* p, bool vec, uint32_t cnt, const uint32_t v[12]) {
  if (vec) {
    uint32_t d[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 12; ++j) d[j / 4] |= v[j] << (8 * (j % 4));
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = d[0], q[1] = d[1], q[2] = d[2];
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if ((uint32_t)j < cnt * 3u) p[j] = (uint8_t)v[j];
  }
}

// grid (x: workgroups of one image, y: images), both strided.  SUM: launch 1 (L of the pixels as a contrast slot finds them -> lsum);
// otherwise launch 2 (every slot, dst written).  src and dst may be the same buffer: a thread reads its own four pixels before it writes them.
template <bool SUM>
__global__ __launch_bounds__(kBlock) void k_color_jitter(const uint8_t* src, uint8_t* dst, const rart_jitter_rec* recs, uint32_t* lsum, int n,
                                                         uint32_t hw, int vec) {
  __shared__ uint32_t part[kBlock / 64];
  const uint32_t groups = (hw + 3u) / 4u;
  for (int img = blockIdx.y; img < n; img += gridDim.y) {
    const CjPlan plan = cj_decode(recs[img]);
    if (SUM && plan.contrast_slot < 0) continue;          // uniform over the workgroup
    const int stop = SUM ? plan.contrast_slot : 4;
    uint32_t mean = 0;
    if (!SUM && plan.contrast_slot >= 0) mean = (uint32_t)((2ull * lsum[img] + hw) / (2ull * hw));
    const size_t base = (size_t)img * hw * 3;
    uint32_t sum = 0;
    for (uint32_t q = blockIdx.x * kBlock + threadIdx.x; q < groups; q += gridDim.x * kBlock) {
      const uint32_t cnt = hw - q * 4u < 4u ? hw - q * 4u : 4u;
      uint32_t v[12];
      cj_load(src + base + (size_t)q * 12, vec != 0, cnt, v);
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        if (j < cnt) {
          cj_apply(plan, stop, mean, v[3 * j], v[3 * j + 1], v[3 * j + 2]);
          if (SUM) sum += cj_luma(v[3 * j], v[3 * j + 1], v[3 * j + 2]);
        }
      }
      if (!SUM) cj_store(dst + base + (size_t)q * 12, vec != 0, cnt, v);
    }
    if (SUM) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
      __syncthreads();                                     // the previous image's partial sums have been read
      if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) t += part[k];
        atomicAdd(&lsum[img], t);
      }
    }
  }
}
}  // namespace

int rart_color_jitter_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, const void* params, uint32_t* lsum, rart_stream_t stream) {
  RART_CHECK_ARG(src && dst && params && lsum, "rart_color_jitter_u8: null pointer");
  RART_CHECK_ARG(n > 0 && h > 0 && w > 0, "rart_color_jitter_u8: n, h, w must be positive");
  const uint64_t hw = (uint64_t)h * (uint64_t)w;
  // the luminance sum of one image is a 32-bit word: 2^24 pixels of L = 255 still fit
  RART_CHECK_ARG(hw <= (1ull << 24), "rart_color_jitter_u8: an image of %d x %d is too large (more than 2^24 pixels)", h, w);
  RART_CHECK_ARG((uint64_t)n * hw * 3ull < (1ull << 32), "rart_color_jitter_u8: too many elements for one launch (split the batch)");
  const size_t bytes = (size_t)n * hw * 3;
  const uintptr_t s0 = (uintptr_t)src, s1 = s0 + bytes, d0 = (uintptr_t)dst, d1 = d0 + bytes;
  RART_CHECK_ARG(d0 == s0 || d1 <= s0 || s1 <= d0, "rart_color_jitter_u8: dst must be src itself or must not overlap it (partial overlap)");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(lsum, 0, (size_t)n * sizeof(uint32_t), st) != hipSuccess) {
    rart_set_error("rart_color_jitter_u8: clearing the workspace failed: %s", hipGetErrorString(hipGetLastError()));
    return RART_ERR_HIP;
  }
  const int vec = (s0 % 4 == 0 && d0 % 4 == 0 && hw % 4 == 0) ? 1 : 0;
  const uint32_t groups = (uint32_t)((hw + 3) / 4);
  const int gy = n < 4096 ? n : 4096;
  const uint32_t per_image = (groups + kBlock - 1) / kBlock, cap = (uint32_t)(4096 / gy);
  const dim3 grid(per_image < cap ? per_image : cap, gy);
  const rart_jitter_rec* recs = (const rart_jitter_rec*)params;
  hipLaunchKernelGGL(k_color_jitter<true>, grid, dim3(kBlock), 0, st, src, dst, recs, lsum, n, (uint32_t)hw, vec);
  hipLaunchKernelGGL(k_color_jitter<false>, grid, dim3(kBlock), 0, st, src, dst, recs, lsum, n, (uint32_t)hw, vec);
  RART_CHECK_LAUNCH("rart_color_jitter_u8");
  return RART_OK;
}
