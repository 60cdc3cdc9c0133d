// The one-wave-per-row LayerNorm skeleton, written once for bf16 storage and for hi + lo pair storage (gfx950): the row lives in
// registers as 16-byte vectors (lane l holds vectors l and l + 64: rows of up to 1024 elements, a multiple of 8), so every tensor
// is read once with coalesced 16-byte loads; statistics in fp32, two passes.  Users: k_layernorm / k_layernorm_bwd
// (csrc/row_norm.hip), k_layernorm_bwd_full (csrc/vit_bwd.hip) and, for the 16-byte load / store alone, k_add_pos_cls
// (csrc/vit_aux.hip).  PAIR = false takes the hi pointer only; its lo pointers are never touched.
// The two storages differ in three things, each in ONE place below, and the bits the kernels write depend on all three:
//   * the root: bf16 rsqrtf(var + eps), pair 1.0f / sqrtf(var + eps) (row_rstd);
//   * the packer: bf16 pack8 = software round-to-nearest-even (f2bf), pair split8 = the hardware convert (row_store8); the two
//     treat NaN payloads differently, so st8<false>, which rounds in hardware, is NOT the bf16 store;
//   * non-temporal loads are the caller's choice per operand (row_load's NT), and only the pair loader has them.
#pragma once
#include "rart_common.h"
#include "rart_bf16_helpers.h"

namespace rart_bf16 {
// load_row for a pair: vectors v (< nv) of hi + lo into r[2][8], zeros elsewhere
template <bool NT = false>
__device__ __forceinline__ void load_row_pair(const uint16_t* hi, const uint16_t* lo, int nv, int lane, float r[2][8]) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = lane + 64 * k;
    uint4 qh = make_uint4(0, 0, 0, 0), ql = make_uint4(0, 0, 0, 0);
    if (v < nv) {
      qh = NT ? rart_nt_load16(hi + (size_t)v * 8) : *reinterpret_cast<const uint4*>(hi + (size_t)v * 8);
      ql = NT ? rart_nt_load16(lo + (size_t)v * 8) : *reinterpret_cast<const uint4*>(lo + (size_t)v * 8);
    }
    join8(qh, ql, r[k]);
  }
}
template <bool PAIR, bool NT = false>
__device__ __forceinline__ void row_load(const uint16_t* h, const uint16_t* l, int nv, int lane, float r[2][8]) {
  static_assert(PAIR || !NT, "only the pair loader has a non-temporal form");
  if constexpr (PAIR) load_row_pair<NT>(h, l, nv, lane, r);
  else load_row(h, nv, lane, r);
}

// eight consecutive elements at h + off (pair: of both planes) <-> fp32
template <bool PAIR>
__device__ __forceinline__ void row_load8(const uint16_t* h, const uint16_t* l, size_t off, float* r) {
  if constexpr (PAIR) join8(*reinterpret_cast<const uint4*>(h + off), *reinterpret_cast<const uint4*>(l + off), r);
  else unpack8(*reinterpret_cast<const uint4*>(h + off), r);
}
template <bool PAIR>
__device__ __forceinline__ void row_store8(uint16_t* h, uint16_t* l, size_t off, const float* r) {
  if constexpr (PAIR) {
    uint4 ph, pl;
    split8(r, ph, pl);
    *reinterpret_cast<uint4*>(h + off) = ph;
    *reinterpret_cast<uint4*>(l + off) = pl;
  } else {
    *reinterpret_cast<uint4*>(h + off) = pack8(r);
  }
}

template <bool PAIR>
__device__ __forceinline__ float row_rstd(float var_plus_eps) {
  return PAIR ? 1.0f / sqrtf(var_plus_eps) : rsqrtf(var_plus_eps);
}

// mean and 1 / sqrt(var + eps) of the row in xr (torch's layer_norm: biased variance, eps inside the root).  The order is part of
// the contract: the sum over all 16 slots (padding vectors are zero), / d, the squared deviations of the occupied vectors, / d, + eps
template <bool PAIR>
__device__ __forceinline__ void ln_row_stats(const float xr[2][8], int nv, int lane, int d, float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) s += xr[k][j];
  mean = rart_wave_sum(s) / (float)d;
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (lane + 64 * k < nv) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = xr[k][j] - mean;
        v += t * t;
      }
    }
  rstd = row_rstd<PAIR>(rart_wave_sum(v) / (float)d + eps);
}

// one vector of the LayerNorm backward: dx = rstd (g - mean(g) - xhat mean(g xhat)) [+ rs], g = dy gamma, stored at oh / ol + off.
// The caller loads the residual vector rs (row_load8) when it has one: with rs a local of this function the compiler zero-fills
// it in front of the conditional load, eight more instructions per vector in k_layernorm_bwd_full's row loop.
template <bool PAIR>
__device__ __forceinline__ void ln_store_dx8(const float* g, const float* xhat, float rstd, float mg, float mgx, bool has_res,
                                             const float* rs, uint16_t* oh, uint16_t* ol, size_t off) {
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    r[j] = rstd * (g[j] - mg - xhat[j] * mgx);
    if (has_res) r[j] += rs[j];
  }
  row_store8<PAIR>(oh, ol, off, r);
}
}  // namespace rart_bf16
