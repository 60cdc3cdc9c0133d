// Mixup / CutMix of a training batch for gfx950 (`mixup`, `cutmix` of the solver's config; robustart_amd/train/mixing.py).
//   x01[i]  = the image as fp32 NCHW in [0, 1]: the source itself, or u8 NHWC * (1 / 255) -- torch's
//             u8.permute(0, 3, 1, 2).float().div(255) on the device multiplies by the fp32 reciprocal (api.hip, k_u8_to_unit_nchw)
//   Mixup:    dst[i] = lam * x01[i] + (1 - lam) * x01[perm[i]]          two products and one sum, no contraction: torch's three kernels
//   CutMix:   dst[i] = x01[perm[i]] inside the box [y0, y1) x [x0, x1), x01[i] outside it: a select, only the chosen image is loaded
// Out of place (image i is also somebody's partner).  A streaming kernel: every output element is written once, 16 bytes per store.
// Per image of h x w pixels the launch moves, u8 source: Mixup 2 * 3hw bytes read + 12hw written, CutMix 3hw + 12hw;
// fp32 source: Mixup 24hw + 12hw, CutMix 12hw + 12hw.
//   u8, w % 4 == 0:   a thread owns four horizontally adjacent pixels: 12 source bytes per image read (three dwords), three float4
//                     plane stores
//   fp32, w % 4 == 0: a thread owns four adjacent elements of one plane: one float4 per image read, one float4 store
//   otherwise:        one output element per thread, the same arithmetic
#include "rart_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;

struct MixArgs {
  int h, w, mode;                 // mode 1 Mixup, 2 CutMix
  float lam, one_minus_lam;       // formed in double on the host, rounded once
  int y0, y1, x0, x1;
};

// plain operators under this file's `fp contract(off)`: the rounding intrinsics of the HIP headers are inline functions compiled with the
// default contraction mode, and their product and sum fuse into an fma once inlined
__device__ __forceinline__ float mb_unit(uint32_t byte) { return (float)byte * (1.0f / 255.0f); }
__device__ __forceinline__ float mb_mix(const MixArgs& a, float own, float partner) {
  const float u = a.lam * own, p = a.one_minus_lam * partner;
  return u + p;
}
__device__ __forceinline__ bool mb_in_box(const MixArgs& a, int y, int x) { return y >= a.y0 && y < a.y1 && x >= a.x0 && x < a.x1; }

// the 12 bytes of four NHWC pixels as three dwords -> v[pixel][channel]
__device__ __forceinline__ void mb_ld12(const uint8_t* __restrict__ p, float v[4][3]) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
  const uint32_t d[3] = {q[0], q[1], q[2]};
#pragma unroll
  for (int j = 0; j < 12; ++j) v[j / 3][j % 3] = mb_unit((d[j / 4] >> (8 * (j % 4))) & 255u);
}

// u8 NHWC source, four pixels of one row per thread.  total = n * h * (w / 4) items.
__global__ __launch_bounds__(kBlock) void k_mix_u8_quad(const uint8_t* __restrict__ src, const int32_t* __restrict__ perm,
                                                        float* __restrict__ dst, uint32_t total, MixArgs a) {
  const uint32_t wq = (uint32_t)a.w / 4, h = (uint32_t)a.h;
  const size_t img_bytes = (size_t)a.h * a.w * 3, plane = (size_t)a.h * a.w;
  // the stride loop counts in 64 bits (total may come close to 2^32), an item's index fits 32
  for (uint64_t it = (uint64_t)blockIdx.x * kBlock + threadIdx.x; it < total; it += (uint64_t)gridDim.x * kBlock) {
    const uint32_t i = (uint32_t)it;
    const uint32_t xq = i % wq, t = i / wq, y = t % h, img = t / h;
    const size_t pix = ((size_t)y * a.w + (size_t)xq * 4) * 3;
    const uint8_t* own = src + (size_t)img * img_bytes + pix;
    const uint8_t* par = src + (size_t)perm[img] * img_bytes + pix;
    float o[4][3];
    if (a.mode == 1) {
      float p[4][3];
      mb_ld12(own, o);
      mb_ld12(par, p);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[j][c] = mb_mix(a, o[j][c], p[j][c]);
    } else {
      const int x = (int)xq * 4;
      const bool row_in = (int)y >= a.y0 && (int)y < a.y1;
      const int lo = x > a.x0 ? x : a.x0, hi = x + 4 < a.x1 ? x + 4 : a.x1;       // the box's share of the four pixels: [lo, hi)
      const int inside = row_in && hi > lo ? hi - lo : 0;
      if (inside == 0) {
        mb_ld12(own, o);
      } else if (inside == 4) {
        mb_ld12(par, o);
      } else {                                           // the box's edge crosses the four pixels: each pixel from its own image
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint8_t* s = (x + j >= lo && x + j < hi) ? par : own;
#pragma unroll
          for (int c = 0; c < 3; ++c) o[j][c] = mb_unit(s[j * 3 + c]);
        }
      }
    }
    float* d = dst + (size_t)img * 3 * plane + (size_t)y * a.w + (size_t)xq * 4;
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(d + c * plane) = make_float4(o[0][c], o[1][c], o[2][c], o[3][c]);
  }
}

// fp32 NCHW source, four elements of one plane row per thread.  total = n * 3 * h * (w / 4) items.
__global__ __launch_bounds__(kBlock) void k_mix_f32_quad(const float* __restrict__ src, const int32_t* __restrict__ perm,
                                                         float* __restrict__ dst, uint32_t total, MixArgs a) {
  const uint32_t wq = (uint32_t)a.w / 4, h = (uint32_t)a.h;
  const size_t plane = (size_t)a.h * a.w;
  for (uint64_t it = (uint64_t)blockIdx.x * kBlock + threadIdx.x; it < total; it += (uint64_t)gridDim.x * kBlock) {
    const uint32_t i = (uint32_t)it;
    const uint32_t xq = i % wq, t = i / wq, y = t % h, pc = t / h, c = pc % 3u, img = pc / 3u;
    const size_t off = (size_t)c * plane + (size_t)y * a.w + (size_t)xq * 4;
    const float* own = src + (size_t)img * 3 * plane + off;
    const float* par = src + (size_t)perm[img] * 3 * plane + off;
    float4 o;
    if (a.mode == 1) {
      const float4 u = *reinterpret_cast<const float4*>(own), p = *reinterpret_cast<const float4*>(par);
      o = make_float4(mb_mix(a, u.x, p.x), mb_mix(a, u.y, p.y), mb_mix(a, u.z, p.z), mb_mix(a, u.w, p.w));
    } else {
      const int x = (int)xq * 4;
      const bool row_in = (int)y >= a.y0 && (int)y < a.y1;
      const int lo = x > a.x0 ? x : a.x0, hi = x + 4 < a.x1 ? x + 4 : a.x1;
      const int inside = row_in && hi > lo ? hi - lo : 0;
      if (inside == 0) {
        o = *reinterpret_cast<const float4*>(own);
      } else if (inside == 4) {
        o = *reinterpret_cast<const float4*>(par);
      } else {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ((x + j >= lo && x + j < hi) ? par : own)[j];
        o = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    *reinterpret_cast<float4*>(dst + (size_t)img * 3 * plane + off) = o;
  }
}

// any width / alignment: one output element per thread.  total = n * 3 * h * w items.
template <bool SRC_U8>
__global__ __launch_bounds__(kBlock) void k_mix_scalar(const void* __restrict__ src, const int32_t* __restrict__ perm, float* __restrict__ dst,
                                                       uint32_t total, MixArgs a) {
  const uint32_t w = (uint32_t)a.w, h = (uint32_t)a.h;
  const size_t plane = (size_t)a.h * a.w;
  for (uint64_t it = (uint64_t)blockIdx.x * kBlock + threadIdx.x; it < total; it += (uint64_t)gridDim.x * kBlock) {
    const uint32_t i = (uint32_t)it;
    const uint32_t x = i % w, t = i / w, y = t % h, pc = t / h, c = pc % 3u, img = pc / 3u;
    const size_t pix = (size_t)y * w + x;
    auto load = [&](uint32_t im) -> float {
      return SRC_U8 ? mb_unit(((const uint8_t*)src)[((size_t)im * plane + pix) * 3 + c])
                    : ((const float*)src)[((size_t)im * 3 + c) * plane + pix];
    };
    float o;
    if (a.mode == 1) {
      const float u = load(img), p = load((uint32_t)perm[img]);
      o = mb_mix(a, u, p);
    } else {
      o = load(mb_in_box(a, (int)y, (int)x) ? (uint32_t)perm[img] : img);
    }
    dst[i] = o;
  }
}
}  // namespace

int rart_mix_batch_f32(const void* src, int src_is_u8, const int32_t* perm, float* dst, int n, int h, int w, int mode, double lam, int y0,
                       int y1, int x0, int x1, rart_stream_t stream) {
  RART_CHECK_ARG(src && perm && dst, "rart_mix_batch_f32: null pointer");
  RART_CHECK_ARG(n > 0 && h > 0 && w > 0, "rart_mix_batch_f32: n, h, w must be positive");
  RART_CHECK_ARG(mode == 1 || mode == 2, "rart_mix_batch_f32: mode must be 1 (Mixup) or 2 (CutMix), got %d", mode);
  RART_CHECK_ARG(lam >= 0.0 && lam <= 1.0, "rart_mix_batch_f32: lam must be in [0, 1]");
  RART_CHECK_ARG(0 <= y0 && y0 <= y1 && y1 <= h && 0 <= x0 && x0 <= x1 && x1 <= w,
                 "rart_mix_batch_f32: the box [%d, %d) x [%d, %d) does not lie inside the %d x %d image", y0, y1, x0, x1, h, w);
  const size_t elems = (size_t)n * 3 * h * w;
  RART_CHECK_ARG(elems < (1ull << 32), "rart_mix_batch_f32: too many elements for one launch (split the batch)");
  const uintptr_t s0 = (uintptr_t)src, s1 = s0 + elems * (src_is_u8 ? 1 : 4), d0 = (uintptr_t)dst, d1 = d0 + elems * 4;
  RART_CHECK_ARG(d1 <= s0 || s1 <= d0, "rart_mix_batch_f32: dst must not overlap src (the launch is out of place)");
  MixArgs a{h, w, mode, (float)lam, (float)(1.0 - lam), y0, y1, x0, x1};
  hipStream_t st = (hipStream_t)stream;
  const bool quad = w % 4 == 0 && d0 % 16 == 0 && s0 % (src_is_u8 ? 4 : 16) == 0;
  if (quad && src_is_u8) {
    const size_t total = elems / 12;
    hipLaunchKernelGGL(k_mix_u8_quad, dim3(rart_grid_for(total, kBlock, 256 * 16)), dim3(kBlock), 0, st, (const uint8_t*)src, perm, dst,
                       (uint32_t)total, a);
  } else if (quad) {
    const size_t total = elems / 4;
    hipLaunchKernelGGL(k_mix_f32_quad, dim3(rart_grid_for(total, kBlock, 256 * 16)), dim3(kBlock), 0, st, (const float*)src, perm, dst,
                       (uint32_t)total, a);
  } else if (src_is_u8) {
    hipLaunchKernelGGL(k_mix_scalar<true>, dim3(rart_grid_for(elems, kBlock, 256 * 16)), dim3(kBlock), 0, st, src, perm, dst,
                       (uint32_t)elems, a);
  } else {
    hipLaunchKernelGGL(k_mix_scalar<false>, dim3(rart_grid_for(elems, kBlock, 256 * 16)), dim3(kBlock), 0, st, src, perm, dst,
                       (uint32_t)elems, a);
  }
  RART_CHECK_LAUNCH("rart_mix_batch_f32");
  return RART_OK;
}
