// Fragment helpers of the fused attention kernels on [token][72] LDS images (head_dim 64, v_mfma_f32_32x32x16_bf16): shared by the
// resident pair kernels (csrc/vit_pair.hip) and the streaming kernels of both storages (csrc/vit_stream.hip), so that what a wave
// computes on a 32-row tile is the same text in both.  LDS images enter the helpers as plain pointers; they are inlined, so the
// accesses stay ds_ instructions.
#pragma once
#include "rart_bf16_helpers.h"

namespace rart_att {
using namespace rart_bf16;
constexpr int PATT_HD = 64, PATT_LDK = PATT_HD + 8;

// every contraction is three MFMA products: lo.hi + hi.lo + hi.hi
#define RART_MFMA3(ACC, AH, AL, BH, BL)                                   \
  ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AL, BH, ACC, 0, 0, 0);    \
  ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AH, BL, ACC, 0, 0, 0);    \
  ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AH, BH, ACC, 0, 0, 0);

// A-operand fragment of a row-major [t][72] image: row t, channels 16 kb + 8 hh .. + 7
__device__ __forceinline__ bf16x8 patt_row_frag(const uint16_t* s, int t, int kb, int hh) {
  return *reinterpret_cast<const bf16x8*>(s + t * PATT_LDK + kb * 16 + hh * 8);
}
// A-operand fragment of the TRANSPOSE of a row-major [t][72] image: rows = channel d, k = the eight tokens t0 + {0,1,2,3,8,9,10,11}
__device__ __forceinline__ bf16x8 patt_tr_frag(const uint16_t* s, int t0, int d) {
  // round 6: two ds_read_b64_tr_b16 instead of eight 2-byte reads.  A 16-lane group reads a [4 tokens][16 channels] block of the row-major
  // image -- lane a supplies the address of channels 4 (a & 3) .. + 3 of token a >> 2 -- and lane a receives channel a of the four tokens
  // (the mapping csrc/wgrad_direct.hip uses; scratch/r4/probe_tr16.hip prints it).  Callers pass d = 32 nt + (lane & 31) and a t0 that is
  // uniform over a 16-lane group, so a = d & 15 and the group's channel base is d - a.  144-byte rows: 8-byte aligned addresses.
  typedef __attribute__((ext_vector_type(4))) short s16x4;
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const int a = d & 15;
  const uint16_t* p = s + (t0 + (a >> 2)) * PATT_LDK + (d - a) + 4 * (a & 3);
  const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
  const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p + 8 * PATT_LDK));
  const s16x8 r = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
  return __builtin_bit_cast(bf16x8, r);
}
__device__ __forceinline__ void patt_split8(const float* v, bf16x8& hi, bf16x8& lo) {
  uint4 h, l;
  split8(v, h, l);
  hi = *reinterpret_cast<bf16x8*>(&h);
  lo = *reinterpret_cast<bf16x8*>(&l);
}
// the B fragments of one row of a pair in global memory (channels 16 kb + 8 hh .. + 7, kb = 0 .. 3 at gh / gl + off); zeros for a row past T
__device__ __forceinline__ void patt_load_frags(bf16x8 (&bh)[4], bf16x8 (&bl)[4], const uint16_t* gh, const uint16_t* gl, size_t off, bool ok,
                                                int hh) {
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    uint4 vh = make_uint4(0, 0, 0, 0), vl = make_uint4(0, 0, 0, 0);
    if (ok) {
      vh = *reinterpret_cast<const uint4*>(gh + off + kb * 16 + hh * 8);
      vl = *reinterpret_cast<const uint4*>(gl + off + kb * 16 + hh * 8);
    }
    bh[kb] = *reinterpret_cast<bf16x8*>(&vh);
    bl[kb] = *reinterpret_cast<bf16x8*>(&vl);
  }
}
// acc[nt][r] = X[the lane's row][d = nt*32 + (r&3) + 8*(r>>2) + 4*hh]: a lane owns runs of four channels of ITS row -> the value (times
// `mul`: the forward's 1 / sum) split into hi + lo, one 8-byte store per plane; dh / dl: channel 0 of the lane's row in each plane
template <bool SCALED>
__device__ __forceinline__ void patt_store_row(const f32x16 (&acc)[2], float mul, uint16_t* dh, uint16_t* dl, int hh) {
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = SCALED ? acc[nt][4 * g + j] * mul : acc[nt][4 * g + j];
      uint2 vh, vl;
      split4(v, vh, vl);
      *reinterpret_cast<uint2*>(dh + nt * 32 + 8 * g + 4 * hh) = vh;
      *reinterpret_cast<uint2*>(dl + nt * 32 + 8 * g + 4 * hh) = vl;
    }
}
}  // namespace rart_att
