// STREAMING fused multi-head attention for gfx950 (head_dim 64, any token count), forward and backward, in both storages: bf16, and the
// reference precision's hi + lo pairs of bf16 planes.  The resident kernels (k_vit_attention[_bwd], csrc/vit_aux.hip; k_vit_attention*_pair,
// csrc/vit_pair.hip) keep a whole (image, head) item in LDS and stop at 224 tokens; here the operands a wave does not own pass through
// LDS in chunks of 64 rows, so the token count is bounded by the index arithmetic alone.
//
// One workgroup of eight waves per (image, head, block); a block is a run of at most eight 32-row tiles, one per wave, and the blocks of
// an item are balanced by tiles (257 tokens = 9 tiles = 4 + 5, not 8 + 1).  Three kernels, each one text for both storages (SaFrag:
// one plane and one MFMA per product, or two planes and three):
//   forward          a wave owns 32 QUERIES (Q fragments in registers) and walks the K / V chunks with a running maximum and running sum
//                    per query; O is rescaled at every chunk, unconditionally (the factor is exactly 1 when the maximum stood);
//   backward, query  per query block: sweep 1 over the K chunks gives max and 1 / sum, delta = rowsum(dO * O) comes from global memory;
//                    sweep 2 over the K / V chunks forms dP, dS and dQ.  Writes dQ and the statistics (max, 1 / sum, delta);
//   backward, key    a wave owns 32 KEYS (K, V fragments in registers); Q, dO and the statistics stream, dK and dV accumulate in registers.
// The per-tile arithmetic is that of the resident kernels: S^T = K Q^T lands with lane = query, the probabilities go straight back as
// the B operand in the key order the accumulator already has (k_vit_attention's trick), the transposed A operands are gathered from
// the row-major images (patt_tr_frag).  No atomics; every output element is written by one lane from sums in a fixed order, and the
// work of an item does not depend on the batch around it.  Rows past the sequence are never read: they enter as zeros, masked keys
// get probability 0.
#include "rart_common.h"
#include "rart_bf16_helpers.h"
#include "rart_att_frag.h"

namespace {
using namespace rart_bf16;
using namespace rart_att;

constexpr int SA_WAVES = 8, SA_BLOCK = SA_WAVES * 64;
constexpr int SA_CHUNK = 64;                              // rows of a streamed chunk: 64 rows x 8 16-byte pieces = one piece per thread and plane
constexpr int SA_IMG = SA_CHUNK * PATT_LDK;               // elements of one plane's [64][72] image
static_assert(SA_CHUNK * 8 == SA_BLOCK, "one 16-byte piece per thread");

// an MFMA operand fragment in the kernel's storage
template <bool PAIR> struct SaFrag;
template <> struct SaFrag<false> { bf16x8 h; };
template <> struct SaFrag<true> { bf16x8 h, l; };

template <bool PAIR>
__device__ __forceinline__ void sa_mma(f32x16& acc, const SaFrag<PAIR>& a, const SaFrag<PAIR>& b) {
  if constexpr (PAIR) {
    RART_MFMA3(acc, a.h, a.l, b.h, b.l)
  } else {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.h, acc, 0, 0, 0);
  }
}
// fragments of a chunk image (plane 1 follows plane 0 at SA_IMG)
template <bool PAIR>
__device__ __forceinline__ SaFrag<PAIR> sa_row_frag(const uint16_t* s, int t, int kb, int hh) {
  SaFrag<PAIR> f;
  f.h = patt_row_frag(s, t, kb, hh);
  if constexpr (PAIR) f.l = patt_row_frag(s + SA_IMG, t, kb, hh);
  return f;
}
template <bool PAIR>
__device__ __forceinline__ SaFrag<PAIR> sa_tr_frag(const uint16_t* s, int t0, int d) {
  SaFrag<PAIR> f;
  f.h = patt_tr_frag(s, t0, d);
  if constexpr (PAIR) f.l = patt_tr_frag(s + SA_IMG, t0, d);
  return f;
}
// eight fp32 values -> a fragment (bf16: hardware round-to-nearest-even; pair: hi + lo)
template <bool PAIR>
__device__ __forceinline__ SaFrag<PAIR> sa_split8(const float* v) {
  SaFrag<PAIR> f;
  if constexpr (PAIR) {
    patt_split8(v, f.h, f.l);
  } else {
    uint4 p = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    f.h = *reinterpret_cast<bf16x8*>(&p);
  }
  return f;
}
// the B fragments of one row in global memory (channels 16 kb + 8 hh .. + 7 at off); zeros when !ok
template <bool PAIR>
__device__ __forceinline__ void sa_load_frags(SaFrag<PAIR> (&f)[4], const uint16_t* gh, const uint16_t* gl, size_t off, bool ok, int hh) {
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    uint4 vh = make_uint4(0, 0, 0, 0), vl = make_uint4(0, 0, 0, 0);
    if (ok) {
      vh = *reinterpret_cast<const uint4*>(gh + off + kb * 16 + hh * 8);
      if constexpr (PAIR) vl = *reinterpret_cast<const uint4*>(gl + off + kb * 16 + hh * 8);
    }
    f[kb].h = *reinterpret_cast<bf16x8*>(&vh);
    if constexpr (PAIR) f[kb].l = *reinterpret_cast<bf16x8*>(&vl);
  }
}
// acc[nt][r] = X[the lane's row][d = nt*32 + (r&3) + 8*(r>>2) + 4*hh] (times mul) -> 8-byte runs of the lane's own row
template <bool PAIR, bool SCALED>
__device__ __forceinline__ void sa_store_row(const f32x16 (&acc)[2], float mul, uint16_t* dh, uint16_t* dl, int hh) {
  if constexpr (PAIR) {
    patt_store_row<SCALED>(acc, mul, dh, dl, hh);
  } else {
    const float k = SCALED ? mul : 1.f;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<uint2*>(dh + nt * 32 + 8 * g + 4 * hh) =
            make_uint2(pack_bf16x2(acc[nt][4 * g] * k, acc[nt][4 * g + 1] * k), pack_bf16x2(acc[nt][4 * g + 2] * k, acc[nt][4 * g + 3] * k));
  }
}

// ---- a chunk on its way to LDS: rows r0 .. r0 + 63 of one operand (64 channels at element offset `base` of the planes, row stride ld),
//      requested into registers before the current chunk is multiplied and committed after it.  Rows past T are zeros and are not read.
template <bool PAIR> struct SaStage { uint4 v[PAIR ? 2 : 1]; };
template <bool PAIR>
__device__ __forceinline__ void sa_issue(SaStage<PAIR>& st, const uint16_t* gh, const uint16_t* gl, size_t base, int r0, int T, int ld) {
  const int t = r0 + ((int)threadIdx.x >> 3), c = threadIdx.x & 7;
  st.v[0] = make_uint4(0, 0, 0, 0);
  if constexpr (PAIR) st.v[1] = make_uint4(0, 0, 0, 0);
  if (t < T) {
    st.v[0] = *reinterpret_cast<const uint4*>(gh + base + (size_t)t * ld + c * 8);
    if constexpr (PAIR) st.v[1] = *reinterpret_cast<const uint4*>(gl + base + (size_t)t * ld + c * 8);
  }
}
template <bool PAIR>
__device__ __forceinline__ void sa_commit(const SaStage<PAIR>& st, uint16_t* s) {
  const int t = (int)threadIdx.x >> 3, c = threadIdx.x & 7;
  *reinterpret_cast<uint4*>(s + t * PATT_LDK + c * 8) = st.v[0];
  if constexpr (PAIR) *reinterpret_cast<uint4*>(s + SA_IMG + t * PATT_LDK + c * 8) = st.v[1];
}

// the workgroup's place: item = (image, head), blk = its block of the item's 32-row tiles; the wave's tile (or none)
struct SaPlace { int item, b, h, tile; bool active; };
__device__ __forceinline__ SaPlace sa_place(int T, int H, int nblk) {
  SaPlace p;
  p.item = blockIdx.x / nblk;
  const int blk = blockIdx.x - p.item * nblk, ntile = (T + 31) / 32;
  p.b = p.item / H;
  p.h = p.item - p.b * H;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  p.tile = blk * ntile / nblk + wave;                      // balanced: block sizes differ by at most one tile
  p.active = p.tile < (blk + 1) * ntile / nblk;
  return p;
}

// S^T = K Q^T of the two key tiles of the chunk in sK, keys past the sequence at -inf; returns the chunk's maximum for the lane's query
template <bool PAIR>
__device__ __forceinline__ float sa_scores(f32x16 (&sacc)[2], const uint16_t* sK, const SaFrag<PAIR> (&bq)[4], int key0, int T) {
  const int lane = threadIdx.x & 63, hh = lane >> 5, l31 = lane & 31;
  float cm = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[kt][r] = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) sa_mma<PAIR>(sacc[kt], sa_row_frag<PAIR>(sK, kt * 32 + l31, kb, hh), bq[kb]);
    // sacc[kt][r] = q . k for key key0 + kt*32 + (r&3) + 8*(r>>2) + 4*hh of the lane's query
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (key0 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh >= T) sacc[kt][r] = -INFINITY;
      cm = fmaxf(cm, sacc[kt][r]);
    }
  }
  return fmaxf(cm, __shfl_xor(cm, 32, 64));
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------------
template <bool PAIR>
__global__ __launch_bounds__(SA_BLOCK) void k_vit_attention_stream(const uint16_t* __restrict__ qkv_h, const uint16_t* __restrict__ qkv_l,
                                                                   uint16_t* __restrict__ att_h, uint16_t* __restrict__ att_l, int T, int H,
                                                                   int ld, int D, float scale_log2e, int nblk) {
  constexpr int NP = PAIR ? 2 : 1;
  __shared__ __attribute__((aligned(16))) uint16_t sK[NP * SA_IMG];
  __shared__ __attribute__((aligned(16))) uint16_t sV[NP * SA_IMG];
  const SaPlace pl = sa_place(T, H, nblk);
  const int lane = threadIdx.x & 63, hh = lane >> 5, l31 = lane & 31;
  const size_t boff = (size_t)pl.b * T * ld + pl.h * PATT_HD;
  const int q = pl.tile * 32 + l31;
  const bool q_ok = pl.active && q < T;
  SaFrag<PAIR> bq[4];
  sa_load_frags<PAIR>(bq, qkv_h, qkv_l, boff + (size_t)q * ld, q_ok, hh);
  f32x16 o[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[nt][r] = 0.f;
  float m = -INFINITY, sum = 0.f;                          // running maximum (raw scores) and the lane's half of the running sum
  const int nchunk = (T + SA_CHUNK - 1) / SA_CHUNK;
  SaStage<PAIR> stK, stV;
  sa_issue<PAIR>(stK, qkv_h, qkv_l, boff + D, 0, T, ld);
  sa_issue<PAIR>(stV, qkv_h, qkv_l, boff + 2 * D, 0, T, ld);
  for (int c = 0; c < nchunk; ++c) {
    sa_commit<PAIR>(stK, sK);
    sa_commit<PAIR>(stV, sV);
    __syncthreads();
    if (c + 1 < nchunk) {
      sa_issue<PAIR>(stK, qkv_h, qkv_l, boff + D, (c + 1) * SA_CHUNK, T, ld);
      sa_issue<PAIR>(stV, qkv_h, qkv_l, boff + 2 * D, (c + 1) * SA_CHUNK, T, ld);
    }
    if (pl.active) {
      f32x16 sacc[2];
      const float cm = sa_scores<PAIR>(sacc, sK, bq, c * SA_CHUNK, T);
      // every chunk holds a key of the sequence, so the new maximum is finite; the first chunk's factor is exp2(-inf) = 0
      const float mn = fmaxf(m, cm);
      const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale_log2e);
      const float mneg = -mn * scale_log2e;               // scale > 0: max(s) * scale == max(s * scale)
      m = mn;
      sum *= alpha;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[nt][r] *= alpha;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2) {
          float e[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            e[j] = __builtin_amdgcn_exp2f(fmaf(sacc[kt][8 * kb2 + j], scale_log2e, mneg));
            sum += e[j];
          }
          const SaFrag<PAIR> pb = sa_split8<PAIR>(e);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            sa_mma<PAIR>(o[nt], sa_tr_frag<PAIR>(sV, kt * 32 + 16 * kb2 + 4 * hh, nt * 32 + l31), pb);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();                                       // every wave is done with this chunk before the next one is committed
  }
  sum += __shfl_xor(sum, 32, 64);
  if (q_ok) {
    const size_t ro = ((size_t)pl.b * T + q) * D + pl.h * PATT_HD;
    sa_store_row<PAIR, true>(o, 1.0f / sum, att_h + ro, PAIR ? att_l + ro : att_h, hh);
  }
}

// ---- backward, query side ---------------------------------------------------------------------------------------------------------------
template <bool PAIR>
__global__ __launch_bounds__(SA_BLOCK) void k_vit_attention_bwd_q_stream(const uint16_t* __restrict__ qkv_h, const uint16_t* __restrict__ qkv_l,
                                                                         const uint16_t* __restrict__ o_h, const uint16_t* __restrict__ o_l,
                                                                         const uint16_t* __restrict__ do_h, const uint16_t* __restrict__ do_l,
                                                                         uint16_t* __restrict__ dq_h, uint16_t* __restrict__ dq_l,
                                                                         float4* __restrict__ stats, int T, int H, int ld, int D, float scale,
                                                                         float scale_log2e, int nblk) {
  constexpr int NP = PAIR ? 2 : 1;
  __shared__ __attribute__((aligned(16))) uint16_t sK[NP * SA_IMG];
  __shared__ __attribute__((aligned(16))) uint16_t sV[NP * SA_IMG];
  const SaPlace pl = sa_place(T, H, nblk);
  const int lane = threadIdx.x & 63, hh = lane >> 5, l31 = lane & 31;
  const size_t boff = (size_t)pl.b * T * ld + pl.h * PATT_HD, doff = (size_t)pl.b * T * D + pl.h * PATT_HD;
  const int q = pl.tile * 32 + l31;
  const bool q_ok = pl.active && q < T;
  SaFrag<PAIR> bq[4], bdo[4];
  sa_load_frags<PAIR>(bq, qkv_h, qkv_l, boff + (size_t)q * ld, q_ok, hh);
  sa_load_frags<PAIR>(bdo, do_h, do_l, doff + (size_t)q * D, q_ok, hh);
  // delta_q = sum_d dO[q][d] O[q][d]: a lane sums its half of the channels, one shuffle adds the halves
  float delta = 0.f;
  if (q_ok) {
    const size_t ro = doff + (size_t)q * D + hh * 32;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float ov[8], dv[8];
      if constexpr (PAIR) {
        join8(*reinterpret_cast<const uint4*>(o_h + ro + c * 8), *reinterpret_cast<const uint4*>(o_l + ro + c * 8), ov);
        join8(*reinterpret_cast<const uint4*>(do_h + ro + c * 8), *reinterpret_cast<const uint4*>(do_l + ro + c * 8), dv);
      } else {
        unpack8(*reinterpret_cast<const uint4*>(o_h + ro + c * 8), ov);
        unpack8(*reinterpret_cast<const uint4*>(do_h + ro + c * 8), dv);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) delta = fmaf(ov[j], dv[j], delta);
    }
  }
  delta += __shfl_xor(delta, 32, 64);
  const int nchunk = (T + SA_CHUNK - 1) / SA_CHUNK;
  SaStage<PAIR> stK, stV;
  // ---- sweep 1: the statistics of the soft-max rows
  float m = -INFINITY, sum = 0.f;
  sa_issue<PAIR>(stK, qkv_h, qkv_l, boff + D, 0, T, ld);
  for (int c = 0; c < nchunk; ++c) {
    sa_commit<PAIR>(stK, sK);
    __syncthreads();
    // past the last chunk: the first chunk of sweep 2
    sa_issue<PAIR>(stK, qkv_h, qkv_l, boff + D, c + 1 < nchunk ? (c + 1) * SA_CHUNK : 0, T, ld);
    if (pl.active) {
      f32x16 sacc[2];
      const float cm = sa_scores<PAIR>(sacc, sK, bq, c * SA_CHUNK, T);
      const float mn = fmaxf(m, cm);
      sum *= __builtin_amdgcn_exp2f((m - mn) * scale_log2e);
      const float mneg = -mn * scale_log2e;
      m = mn;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f(fmaf(sacc[kt][r], scale_log2e, mneg));
    }
    __syncthreads();
  }
  sum += __shfl_xor(sum, 32, 64);
  const float ms = m * scale_log2e, inv = 1.0f / sum;
  // all 32 rows of the wave's tile, the ones past the sequence included (finite: their Q rows are zeros): the key side reads whole tiles
  if (pl.active && hh == 0) stats[(size_t)pl.item * (((T + 31) / 32) * 32) + q] = make_float4(ms, inv, delta, 0.f);
  const float sinv = scale * inv;
  // ---- sweep 2: dP^T = V dO^T, dS, dQ^T = K^T dS^T
  f32x16 dq[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[nt][r] = 0.f;
  sa_issue<PAIR>(stV, qkv_h, qkv_l, boff + 2 * D, 0, T, ld);
  for (int c = 0; c < nchunk; ++c) {
    sa_commit<PAIR>(stK, sK);
    sa_commit<PAIR>(stV, sV);
    __syncthreads();
    if (c + 1 < nchunk) {
      sa_issue<PAIR>(stK, qkv_h, qkv_l, boff + D, (c + 1) * SA_CHUNK, T, ld);
      sa_issue<PAIR>(stV, qkv_h, qkv_l, boff + 2 * D, (c + 1) * SA_CHUNK, T, ld);
    }
    if (pl.active) {
      f32x16 sacc[2];
      sa_scores<PAIR>(sacc, sK, bq, c * SA_CHUNK, T);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        f32x16 dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) sa_mma<PAIR>(dp, sa_row_frag<PAIR>(sV, kt * 32 + l31, kb, hh), bdo[kb]);
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2) {
          float dsv[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float e = __builtin_amdgcn_exp2f(fmaf(sacc[kt][8 * kb2 + j], scale_log2e, -ms));      // masked keys: exp2(-inf) = 0
            dsv[j] = sinv * e * (dp[8 * kb2 + j] - delta);
          }
          const SaFrag<PAIR> ds = sa_split8<PAIR>(dsv);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            sa_mma<PAIR>(dq[nt], sa_tr_frag<PAIR>(sK, kt * 32 + 16 * kb2 + 4 * hh, nt * 32 + l31), ds);
        }
        __builtin_amdgcn_sched_barrier(0);                 // one key tile at a time
      }
    }
    __syncthreads();
  }
  // dq[nt][r] = dQ[query q][d = nt*32 + (r&3) + 8*(r>>2) + 4*hh]
  if (q_ok) sa_store_row<PAIR, false>(dq, 1.f, dq_h + boff + (size_t)q * ld, PAIR ? dq_l + boff + (size_t)q * ld : dq_h, hh);
}

// ---- backward, key side -------------------------------------------------------------------------------------------------------------------
template <bool PAIR>
__global__ __launch_bounds__(SA_BLOCK) void k_vit_attention_bwd_kv_stream(const uint16_t* __restrict__ qkv_h, const uint16_t* __restrict__ qkv_l,
                                                                          const uint16_t* __restrict__ do_h, const uint16_t* __restrict__ do_l,
                                                                          uint16_t* __restrict__ dq_h, uint16_t* __restrict__ dq_l,
                                                                          const float4* __restrict__ stats, int T, int H, int ld, int D,
                                                                          float scale, float scale_log2e, int nblk) {
  constexpr int NP = PAIR ? 2 : 1;
  __shared__ __attribute__((aligned(16))) uint16_t sQ[NP * SA_IMG];
  __shared__ __attribute__((aligned(16))) uint16_t sdO[NP * SA_IMG];
  __shared__ __attribute__((aligned(16))) float4 sStat[SA_CHUNK];
  const SaPlace pl = sa_place(T, H, nblk);
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, l31 = lane & 31;
  const size_t boff = (size_t)pl.b * T * ld + pl.h * PATT_HD, doff = (size_t)pl.b * T * D + pl.h * PATT_HD;
  const int TP = ((T + 31) / 32) * 32;
  const float4* const istat = stats + (size_t)pl.item * TP;
  const int key = pl.tile * 32 + l31;
  const bool key_ok = pl.active && key < T;
  SaFrag<PAIR> bk[4], bv[4];
  sa_load_frags<PAIR>(bk, qkv_h, qkv_l, boff + (size_t)key * ld + D, key_ok, hh);
  sa_load_frags<PAIR>(bv, qkv_h, qkv_l, boff + (size_t)key * ld + 2 * D, key_ok, hh);
  // dV^T = dO^T . P and dK^T = Q^T . dS (operands swapped): lane = key, registers = channels
  f32x16 dvv[2], dkk[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dvv[nt][r] = dkk[nt][r] = 0.f;
  const int nchunk = (T + SA_CHUNK - 1) / SA_CHUNK;
  SaStage<PAIR> stQ, stD;
  float4 stS = make_float4(0.f, 0.f, 0.f, 0.f);            // rows past the item's tiles: probability exp2(0 - 0) * 0 = 0
  auto issue = [&](int r0) {
    sa_issue<PAIR>(stQ, qkv_h, qkv_l, boff, r0, T, ld);
    sa_issue<PAIR>(stD, do_h, do_l, doff, r0, T, D);
    if (tid < SA_CHUNK) stS = r0 + tid < TP ? istat[r0 + tid] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  issue(0);
  for (int c = 0; c < nchunk; ++c) {
    sa_commit<PAIR>(stQ, sQ);
    sa_commit<PAIR>(stD, sdO);
    if (tid < SA_CHUNK) sStat[tid] = stS;
    __syncthreads();
    if (c + 1 < nchunk) issue((c + 1) * SA_CHUNK);
    if (pl.active) {
#pragma unroll 1
      for (int qt = 0; qt < 2; ++qt) {
        f32x16 sa, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) sa[r] = dp[r] = 0.f;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
          sa_mma<PAIR>(sa, sa_row_frag<PAIR>(sQ, qt * 32 + l31, kb, hh), bk[kb]);
          sa_mma<PAIR>(dp, sa_row_frag<PAIR>(sdO, qt * 32 + l31, kb, hh), bv[kb]);
        }
        // lane = key; register r = query qt*32 + (r&3) + 8*(r>>2) + 4*hh of the chunk (queries past the sequence have zero Q / dO rows:
        // whatever probability they get multiplies zeros)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float4 st = sStat[qt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh];
          const float pv = key_ok ? __builtin_amdgcn_exp2f(fmaf(sa[r], scale_log2e, -st.x)) * st.y : 0.f;
          sa[r] = pv;
          dp[r] = scale * pv * (dp[r] - st.z);
        }
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2) {
          float pw[8], dw[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            pw[j] = sa[8 * kb2 + j];
            dw[j] = dp[8 * kb2 + j];
          }
          const SaFrag<PAIR> pb = sa_split8<PAIR>(pw), db = sa_split8<PAIR>(dw);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            const int t0 = qt * 32 + 16 * kb2 + 4 * hh, dch = nt * 32 + l31;
            sa_mma<PAIR>(dvv[nt], sa_tr_frag<PAIR>(sdO, t0, dch), pb);
            sa_mma<PAIR>(dkk[nt], sa_tr_frag<PAIR>(sQ, t0, dch), db);
          }
        }
      }
    }
    __syncthreads();
  }
  // dkk / dvv[nt][r] = dK / dV[key][d = nt*32 + (r&3) + 8*(r>>2) + 4*hh]: 8-byte runs of the lane's own key row
  if (key_ok) {
    const size_t ro = boff + (size_t)key * ld;
    sa_store_row<PAIR, false>(dkk, 1.f, dq_h + ro + D, PAIR ? dq_l + ro + D : dq_h, hh);
    sa_store_row<PAIR, false>(dvv, 1.f, dq_h + ro + 2 * D, PAIR ? dq_l + ro + 2 * D : dq_h, hh);
  }
}
#undef RART_MFMA3

// blocks per item: runs of at most SA_WAVES tiles.  0 (and the error string) when the launch grid or the 32-bit tile arithmetic of
// the kernels cannot hold the shape
int sa_blocks(const char* who, int n, int tokens, int heads) {
  const long long ntile = ((long long)tokens + 31) / 32, nblk = (ntile + SA_WAVES - 1) / SA_WAVES;
  if (tokens > (1 << 20) || heads > 0x7fffffff / 3 / PATT_HD || (long long)n * heads * nblk > 0x7fffffffll) {
    rart_set_error("%s: n = %d, tokens = %d, heads = %d is more than the kernel's 32-bit indices hold", who, n, tokens, heads);
    return 0;
  }
  return (int)nblk;
}

template <bool PAIR>
int sa_forward(const char* who, const void* qh, const void* ql, void* oh, void* ol, int n, int tokens, int heads, rart_stream_t stream) {
  const int nblk = sa_blocks(who, n, tokens, heads);
  if (!nblk) return RART_ERR_INVALID;
  const int D = heads * PATT_HD;
  const float scale_log2e = (1.0f / sqrtf((float)PATT_HD)) * 1.4426950408889634f;
  hipLaunchKernelGGL(k_vit_attention_stream<PAIR>, dim3((uint32_t)(n * heads * nblk)), dim3(SA_BLOCK), 0, (hipStream_t)stream,
                     (const uint16_t*)qh, (const uint16_t*)ql, (uint16_t*)oh, (uint16_t*)ol, tokens, heads, 3 * D, D, scale_log2e, nblk);
  RART_CHECK_LAUNCH(who);
  return RART_OK;
}

template <bool PAIR>
int sa_backward(const char* who, const void* qh, const void* ql, const void* oh, const void* ol, const void* dh, const void* dl, void* gh,
                void* gl, float* stats, int n, int tokens, int heads, rart_stream_t stream) {
  const int nblk = sa_blocks(who, n, tokens, heads);
  if (!nblk) return RART_ERR_INVALID;
  const int D = heads * PATT_HD;
  const float scale = 1.0f / sqrtf((float)PATT_HD), sl2e = scale * 1.4426950408889634f;
  const dim3 grid((uint32_t)(n * heads * nblk));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_vit_attention_bwd_q_stream<PAIR>, grid, dim3(SA_BLOCK), 0, st, (const uint16_t*)qh, (const uint16_t*)ql,
                     (const uint16_t*)oh, (const uint16_t*)ol, (const uint16_t*)dh, (const uint16_t*)dl, (uint16_t*)gh, (uint16_t*)gl,
                     (float4*)stats, tokens, heads, 3 * D, D, scale, sl2e, nblk);
  hipLaunchKernelGGL(k_vit_attention_bwd_kv_stream<PAIR>, grid, dim3(SA_BLOCK), 0, st, (const uint16_t*)qh, (const uint16_t*)ql,
                     (const uint16_t*)dh, (const uint16_t*)dl, (uint16_t*)gh, (uint16_t*)gl, (const float4*)stats, tokens, heads, 3 * D, D,
                     scale, sl2e, nblk);
  RART_CHECK_LAUNCH(who);
  return RART_OK;
}
}  // namespace

extern "C" {

int rart_vit_attention_stream(const void* qkv, void* out, int n, int tokens, int heads, int head_dim, rart_stream_t stream) {
  RART_CHECK_ARG(qkv && out && n > 0 && tokens >= 1 && heads > 0, "rart_vit_attention_stream: bad arguments");
  RART_CHECK_ARG(head_dim == 64, "rart_vit_attention_stream: head_dim must be 64");
  return sa_forward<false>("rart_vit_attention_stream", qkv, nullptr, out, nullptr, n, tokens, heads, stream);
}

int rart_vit_attention_bwd_stream(const void* qkv, const void* out, const void* dout, void* dqkv, float* stats, int n, int tokens, int heads,
                                  int head_dim, rart_stream_t stream) {
  RART_CHECK_ARG(qkv && out && dout && dqkv && stats && n > 0 && tokens >= 1 && heads > 0, "rart_vit_attention_bwd_stream: bad arguments");
  RART_CHECK_ARG(head_dim == 64, "rart_vit_attention_bwd_stream: head_dim must be 64");
  return sa_backward<false>("rart_vit_attention_bwd_stream", qkv, nullptr, out, nullptr, dout, nullptr, dqkv, nullptr, stats, n, tokens, heads,
                            stream);
}

int rart_vit_attention_stream_pair(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, int n, int tokens, int heads,
                                   int head_dim, rart_stream_t stream) {
  RART_CHECK_ARG(qkv_hi && qkv_lo && out_hi && out_lo && n > 0 && tokens >= 1 && heads > 0, "rart_vit_attention_stream_pair: bad arguments");
  RART_CHECK_ARG(head_dim == 64, "rart_vit_attention_stream_pair: head_dim must be 64");
  return sa_forward<true>("rart_vit_attention_stream_pair", qkv_hi, qkv_lo, out_hi, out_lo, n, tokens, heads, stream);
}

int rart_vit_attention_bwd_stream_pair(const void* qkv_hi, const void* qkv_lo, const void* out_hi, const void* out_lo, const void* dout_hi,
                                       const void* dout_lo, void* dqkv_hi, void* dqkv_lo, float* stats, int n, int tokens, int heads,
                                       int head_dim, rart_stream_t stream) {
  RART_CHECK_ARG(qkv_hi && qkv_lo && out_hi && out_lo && dout_hi && dout_lo && dqkv_hi && dqkv_lo && stats && n > 0 && tokens >= 1 && heads > 0,
                 "rart_vit_attention_bwd_stream_pair: bad arguments");
  RART_CHECK_ARG(head_dim == 64, "rart_vit_attention_bwd_stream_pair: head_dim must be 64");
  return sa_backward<true>("rart_vit_attention_bwd_stream_pair", qkv_hi, qkv_lo, out_hi, out_lo, dout_hi, dout_lo, dqkv_hi, dqkv_lo, stats, n,
                           tokens, heads, stream);
}

}  // extern "C"
