// bf16 and split-bf16 (hi + lo pair) element helpers shared by every kernel file that touches bf16 storage (gfx950): conversions,
// 2- / 8-wide packing, pair split / join, 8-channel loads and stores, and the 1-bit ReLU-mask helpers of the fused convolutions.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;   // (arrays of HIP's uint4 struct end up in scratch; ext vectors do not)

namespace rart_bf16 {
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) short i16x2_t;
// the 16 bits of a bf16 -> float, and float -> bf16 bits by software round-to-nearest-even (finite inputs)
__device__ __forceinline__ float bf2f(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
// two floats -> packed bf16 pair, hardware round-to-nearest-even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  f32x2_t f = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2_t));
}
// ReLU on a packed pair with 16-bit integer ops (a bf16 is > 0 exactly when its bits, read as int16, are > 0)
__device__ __forceinline__ uint32_t relu_bf16x2(uint32_t w) {
  const i16x2_t z = {0, 0};
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(i16x2_t, w), z));
}
// bits (2*pair, 2*pair+1) of `byte` -> 0xFFFF / 0 halves
__device__ __forceinline__ uint32_t halves_from_bits(uint32_t byte, uint32_t pair) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_sbfe(byte, 2u * pair, 1u);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_sbfe(byte, 2u * pair + 1u, 1u);
  return __builtin_amdgcn_perm(hi, lo, 0x07060100u);
}
// a packed bf16 pair -> 2 bits (value > 0)
__device__ __forceinline__ uint32_t bits_from_halves(uint32_t w) {
  const i16x2_t z = {0, 0}, one = {1, 1};
  const uint32_t t = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_elementwise_max(__builtin_bit_cast(i16x2_t, w), z), one));
  return (t | (t >> 15)) & 3u;
}
// eight packed bf16 values -> their sign byte (bit j = value j > 0)
__device__ __forceinline__ uint32_t sign_byte(uint4 v) {
  return bits_from_halves(v.x) | (bits_from_halves(v.y) << 2) | (bits_from_halves(v.z) << 4) | (bits_from_halves(v.w) << 6);
}

// ---- eight bf16 values in one 16-byte vector <-> fp32 (software RNE on the way back)
__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = __uint_as_float(w[j] << 16);
    f[2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u);
  }
}
__device__ __forceinline__ uint4 pack8(const float* f) {
  return make_uint4(f2bf(f[0]) | ((uint32_t)f2bf(f[1]) << 16), f2bf(f[2]) | ((uint32_t)f2bf(f[3]) << 16),
                    f2bf(f[4]) | ((uint32_t)f2bf(f[5]) << 16), f2bf(f[6]) | ((uint32_t)f2bf(f[7]) << 16));
}
// one wave per row, lane l holds the row's 16-byte vectors l and l + 64: loads vectors v (< nv) into r[2][8] (zeros elsewhere)
__device__ __forceinline__ void load_row(const uint16_t* row, int nv, int lane, float r[2][8]) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = lane + 64 * k;
    uint4 q = make_uint4(0, 0, 0, 0);
    if (v < nv) q = *reinterpret_cast<const uint4*>(row + (size_t)v * 8);
    unpack8(q, r[k]);
  }
}

// ---- pairs: value = hi + lo with hi = bf16(v), lo = bf16(v - hi), hardware RNE; hi + lo is exact in fp32 (two 8-bit significands, lo
//      below half an ulp of hi)
__device__ __forceinline__ void split8(const float* v, uint4& hi, uint4& lo) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    h[j] = pack_bf16x2(v[2 * j], v[2 * j + 1]);
    l[j] = pack_bf16x2(v[2 * j] - __uint_as_float(h[j] << 16), v[2 * j + 1] - __uint_as_float(h[j] & 0xFFFF0000u));
  }
  hi = make_uint4(h[0], h[1], h[2], h[3]);
  lo = make_uint4(l[0], l[1], l[2], l[3]);
}
__device__ __forceinline__ void split4(const float* v, uint2& hi, uint2& lo) {
  const uint32_t h0 = pack_bf16x2(v[0], v[1]), h1 = pack_bf16x2(v[2], v[3]);
  hi = make_uint2(h0, h1);
  lo = make_uint2(pack_bf16x2(v[0] - __uint_as_float(h0 << 16), v[1] - __uint_as_float(h0 & 0xFFFF0000u)),
                  pack_bf16x2(v[2] - __uint_as_float(h1 << 16), v[3] - __uint_as_float(h1 & 0xFFFF0000u)));
}
__device__ __forceinline__ void join4(const uint2& hi, const uint2& lo, float* v) {
  v[0] = __uint_as_float(hi.x << 16) + __uint_as_float(lo.x << 16);
  v[1] = __uint_as_float(hi.x & 0xFFFF0000u) + __uint_as_float(lo.x & 0xFFFF0000u);
  v[2] = __uint_as_float(hi.y << 16) + __uint_as_float(lo.y << 16);
  v[3] = __uint_as_float(hi.y & 0xFFFF0000u) + __uint_as_float(lo.y & 0xFFFF0000u);
}
__device__ __forceinline__ void join8(const uint4& hi, const uint4& lo, float* v) {
  const uint32_t h[4] = {hi.x, hi.y, hi.z, hi.w}, l[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = __uint_as_float(h[j] << 16) + __uint_as_float(l[j] << 16);
    v[2 * j + 1] = __uint_as_float(h[j] & 0xFFFF0000u) + __uint_as_float(l[j] & 0xFFFF0000u);
  }
}

// ---- eight consecutive elements at h + i of a bf16 tensor, or (PAIR) of the hi / lo planes h, l: one 16-byte access per plane.  The
//      forms below (lo plane added in place; st8 splitting even when only hi is stored) are the ones that leave the generated code of
//      both users, convnext_v2.hip and convstem.hip, as it was with their own copies
template <bool PAIR>
__device__ __forceinline__ void ld8(const uint16_t* __restrict__ h, const uint16_t* __restrict__ l, size_t i, float* v) {
  unpack8(*reinterpret_cast<const uint4*>(h + i), v);
  if (PAIR) {
    const uint4 b = *reinterpret_cast<const uint4*>(l + i);
    const uint32_t bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] += __uint_as_float(bw[j] << 16);
      v[2 * j + 1] += __uint_as_float(bw[j] & 0xFFFF0000u);
    }
  }
}
template <bool PAIR>
__device__ __forceinline__ void st8(uint16_t* __restrict__ h, uint16_t* __restrict__ l, size_t i, const float* v) {
  uint4 hi, lo;
  split8(v, hi, lo);
  *reinterpret_cast<uint4*>(h + i) = hi;
  if (PAIR) *reinterpret_cast<uint4*>(l + i) = lo;
}
}  // namespace rart_bf16
