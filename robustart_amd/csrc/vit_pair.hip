// Non-GEMM kernels of the REFERENCE-PRECISION ("fp32x" / "bf16x3") ViT-B/16 engine for gfx950: every activation and gradient is a
// PAIR of bf16 planes (value = hi + lo, 16 significand bits; exact in fp32), every contraction runs on rart_gemm_pair_bf16
// (csrc/gemm_pair.hip), and what is left here -- the attention soft-max rows and their backward -- are the HBM-bound row kernels
// below: read the pair, compute in fp32 exactly as the fp32 module does (max-subtracted soft-max with libm's expf), write the pair.
// (LayerNorm forward and backward-to-input: csrc/row_norm.hip; the class-token / position add: csrc/vit_aux.hip.)  The reference runs
// ViT in fp32 (exprs/exp/imagenet_c_loop_mini/config_vit_base.yaml:1-9: no precision key; adv/attack.py:20-23; autopgd_base.py:271-289); model
// `vit_base` = timm ViT-B/16 (RobustART/model/__init__.py:1 -> absent submodule; robustart_amd/model/vit_torch.py).
#include "rart_common.h"
#include "rart_bf16_helpers.h"
#include <stdlib.h>
#include "rart_lds_dma.h"
#include "rart_att_frag.h"

namespace {
using namespace rart_bf16;
using namespace rart_att;
constexpr int kBlock = 256;

// P[row][0..n_valid) = softmax(scale * S[row][0..n_valid)) as a pair, P[row][n_valid..ld_out) = 0; S fp32 (the pair GEMM's fp32
// output).  One wave per row, four consecutive columns per lane (rows of up to 256 columns)
__global__ __launch_bounds__(kBlock) void k_softmax_rows_pair(const float* __restrict__ sm, uint16_t* __restrict__ ph,
                                                              uint16_t* __restrict__ pl, long long rows, int n_valid, int ld_in,
                                                              int ld_out, float scale) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int c0 = lane * 4;
  float4 sv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c0 < ld_in) sv = *reinterpret_cast<const float4*>(sm + row * ld_in + c0);
  float s[4] = {sv.x, sv.y, sv.z, sv.w};
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (c0 + j < n_valid) mx = fmaxf(mx, s[j] * scale);
  mx = rart_wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s[j] = (c0 + j < n_valid) ? expf(s[j] * scale - mx) : 0.f;
    sum += s[j];
  }
  sum = rart_wave_sum(sum);
  if (c0 < ld_out) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = s[j] / sum;
    uint2 oh, ol;
    split4(s, oh, ol);
    *reinterpret_cast<uint2*>(ph + row * ld_out + c0) = oh;
    *reinterpret_cast<uint2*>(pl + row * ld_out + c0) = ol;
  }
}

// dS[row][c] = scale * P[row][c] * (dP[row][c] - sum_k P[row][k] dP[row][k]), c < n_valid; zeros up to ld_out.  P pair, dP fp32.
__global__ __launch_bounds__(kBlock) void k_softmax_bwd_rows_pair(const uint16_t* __restrict__ ph, const uint16_t* __restrict__ pl,
                                                                  const float* __restrict__ dp, uint16_t* __restrict__ dh,
                                                                  uint16_t* __restrict__ dl, long long rows, int n_valid, int ld_p,
                                                                  int ld_dp, int ld_out, float scale) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int c0 = lane * 4;
  float p[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f};
  if (c0 < ld_p) join4(*reinterpret_cast<const uint2*>(ph + row * ld_p + c0), *reinterpret_cast<const uint2*>(pl + row * ld_p + c0), p);
  if (c0 < ld_dp) {
    const float4 gv = *reinterpret_cast<const float4*>(dp + row * ld_dp + c0);
    g[0] = gv.x; g[1] = gv.y; g[2] = gv.z; g[3] = gv.w;
  }
  float dot = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (c0 + j < n_valid) dot += p[j] * g[j];
  dot = rart_wave_sum(dot);
  if (c0 < ld_out) {
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = (c0 + j < n_valid) ? scale * p[j] * (g[j] - dot) : 0.f;
    uint2 oh, ol;
    split4(r, oh, ol);
    *reinterpret_cast<uint2*>(dh + row * ld_out + c0) = oh;
    *reinterpret_cast<uint2*>(dl + row * ld_out + c0) = ol;
  }
}

// ---- fused multi-head attention on pairs (head_dim 64, tokens <= NKT*32): forward, backward-q and backward-kv, each as a ONE-ITEM kernel
//      (one workgroup per (image, head)) and as a WALKING kernel (round 6: one workgroup per CU takes a run of items, wave 7 loads the next
//      item's operands by LDS-DMA while the other seven compute).  The two forms of a family differ in how the operands reach LDS and in
//      where the workgroup barriers stand; what a wave computes on a 32-row tile is the SAME text, the patt_* helpers below, so the two
//      forms agree bit for bit by construction (tests/test_vit_x3_gpu.py compares them, tests/test_att_pair_bits_gpu.py holds both to a
//      recording).  The fragment helpers (patt_row_frag, patt_tr_frag, patt_split8, patt_load_frags, patt_store_row, RART_MFMA3) are in
//      rart_att_frag.h, which the streaming kernels (csrc/vit_stream.hip) share.
// Round 6: EIGHT waves per workgroup (512 threads) instead of four.  The LDS images keep these kernels at one workgroup per CU, so with four
// waves every SIMD held ONE wave -- nothing ran beside its soft-max VALU work, its LDS gathers or its K / V staging, the matrix pipes were
// busy 12-13 % of a launch (profiles/r05_x3_counters.json) -- and the seven 32-query tiles of ViT-B/16's 197 tokens took two rounds over
// four waves.  With eight waves the seven tiles run in one round, two waves per SIMD, and one wave's MFMAs cover the other's vector work.
constexpr int kAttBlock = 512;
constexpr int PATT_MAX_TILES = kAttBlock / 64 - 1;       // 224 tokens: every 32-row tile of an item has a wave of its own; the walking kernels' wave 7 loads

// one plane of an operand into a row-major [t][72] LDS image, rows past T zero (the one-item kernels' staging)
__device__ __forceinline__ void patt_load_rows(uint16_t* s, const uint16_t* g, int T, int TP, int ld, int tid) {
  for (int i = tid; i < TP * 8; i += kAttBlock) {                         // [t][72]: 16-byte chunks, coalesced
    const int t = i >> 3, c = i & 7;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (t < T) v = *reinterpret_cast<const uint4*>(g + (size_t)t * ld + c * 8);
    *reinterpret_cast<uint4*>(s + t * PATT_LDK + c * 8) = v;
  }
}

// ---- what the walking kernels share
// element offset of item `it`'s (image, head) block inside a plane of row stride ld
__device__ __forceinline__ size_t patt_item_base(int it, int H, int T, int ld) {
  const int b = it / H;
  return (size_t)b * T * ld + (it - b * H) * PATT_HD;
}
// a workgroup barrier that also orders the LDS traffic around it: the loader wave's DMA and the compute waves' reads meet here
__device__ __forceinline__ void patt_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// the LDS byte address of an image, as the DMA's M0 wants it.  (The loaders' DMA loops stay per kernel: one shared helper for "instructions
// i0 .. i1 of a padded image, hi and lo plane" compiled to other loader-wave code -- 27 to 190 more instructions -- whichever way it was written.)
#define PATT_LDS_ADDR(A) ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t*)&(A))

// ---- forward ------------------------------------------------------------------------------------------------------------------------------
// The structure of k_vit_attention (csrc/vit_aux.hip) with every contraction as three MFMA products: K_hi / K_lo rows and V_hi / V_lo
// are resident in LDS, a wave owns 32 queries; S^T = K Q^T lands with lane (l & 31) = the QUERY, so the soft-max statistics of a query
// live in one lane pair and the whole score row stays in registers (fp32, as the fp32 module computes it); the un-normalised
// probabilities e = exp(s - max) are split into hi + lo and fed straight back as the B operand of O^T = V^T P^T in the key order the
// accumulator registers already have; O is scaled by 1 / sum and written as a pair.
// Replaces, per layer and forward pass, the batched S = Q K^T product (fp32 scores, 0.5 GB at B = 256), the soft-max row kernel, two
// V transposes and the batched P V product of the unfused path (ViTEngine.fused_attention = False keeps that path as the cross-check).

// sacc[kt] = (K Q^T)[key tile kt] for kt < NKT from the K image and the wave's Q fragments (also the backward-q's S).  BARRIER_LAST: a
// workgroup barrier in front of the last key tile (the walking backward-q's A6)
template <int NKT, bool BARRIER_LAST>
__device__ __forceinline__ void patt_scores(f32x16 (&sacc)[NKT], const uint16_t* kh, const uint16_t* kl, const bf16x8 (&bh)[4],
                                            const bf16x8 (&bl)[4]) {
  const int lane = threadIdx.x & 63, hh = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    if (BARRIER_LAST && kt == NKT - 1) patt_barrier();
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[kt][r] = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const bf16x8 ah = patt_row_frag(kh, kt * 32 + l31, kb, hh), al = patt_row_frag(kl, kt * 32 + l31, kb, hh);
      RART_MFMA3(sacc[kt], ah, al, bh[kb], bl[kb])
    }
    __builtin_amdgcn_sched_barrier(0);          // keep the K fragments of later key tiles out of the register file
  }
}
// Where the A fragment of O^T = V^T P^T (rows = channel d, k = the eight tokens t0 + {0,1,2,3,8,9,10,11}) comes from.  The one-item
// kernel transposes V on the way in: [channel][LDV] rows, two 8-byte reads.  The walking kernel's DMA cannot transpose: its V image is
// row-major and the fragment is gathered by patt_tr_frag, as in the backward kernels.
template <int LDV>
struct PattVTransposed {
  const uint16_t* s[2];
  __device__ __forceinline__ bf16x8 frag(int p, int t0, int d) const {
    const uint2 v0 = *reinterpret_cast<const uint2*>(s[p] + d * LDV + t0), v1 = *reinterpret_cast<const uint2*>(s[p] + d * LDV + t0 + 8);
    uint4 v = make_uint4(v0.x, v0.y, v1.x, v1.y);
    return *reinterpret_cast<bf16x8*>(&v);
  }
};
struct PattVRowMajor {
  const uint16_t* s[2];
  __device__ __forceinline__ bf16x8 frag(int p, int t0, int d) const { return patt_tr_frag(s[p], t0, d); }
};
// soft-max over the score row in sacc and o = the un-normalised O^T = V^T P^T; returns 1 / sum.  SCHED_PER_KB2: a sched_barrier after
// every 16 keys (the walking kernel) instead of after every key tile (the one-item kernel) -- each form keeps the placement it was tuned with.
template <int NKT, bool SCHED_PER_KB2, class VSource>
__device__ __forceinline__ float patt_softmax_pv(f32x16 (&sacc)[NKT], f32x16 (&o)[2], const VSource& vs, int T, float scale_log2e) {
  const int lane = threadIdx.x & 63, hh = lane >> 5, l31 = lane & 31;
  // sacc[kt][r] = q . k for key kt*32 + (r&3) + 8*(r>>2) + 4*hh of query q.  Keys past the sequence must not win the maximum: only
  // the LAST key tile can hold any (the host picks NKT = ceil(T / 32))
  float m = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if ((NKT - 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh >= T) sacc[NKT - 1][r] = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, sacc[kt][r]);
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  const float mneg = -m * scale_log2e;            // scale > 0: max(s) * scale == max(s * scale)
  float sum = 0.f;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[nt][r] = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    uint32_t ph[8], pl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float e0 = __builtin_amdgcn_exp2f(fmaf(sacc[kt][2 * j], scale_log2e, mneg));
      const float e1 = __builtin_amdgcn_exp2f(fmaf(sacc[kt][2 * j + 1], scale_log2e, mneg));
      sum += e0 + e1;
      ph[j] = pack_bf16x2(e0, e1);
      pl[j] = pack_bf16x2(e0 - __uint_as_float(ph[j] << 16), e1 - __uint_as_float(ph[j] & 0xFFFF0000u));
    }
#pragma unroll
    for (int kb2 = 0; kb2 < 2; ++kb2) {
      uint4 pvh = make_uint4(ph[4 * kb2], ph[4 * kb2 + 1], ph[4 * kb2 + 2], ph[4 * kb2 + 3]);
      uint4 pvl = make_uint4(pl[4 * kb2], pl[4 * kb2 + 1], pl[4 * kb2 + 2], pl[4 * kb2 + 3]);
      const bf16x8 pbh = *reinterpret_cast<bf16x8*>(&pvh), pbl = *reinterpret_cast<bf16x8*>(&pvl);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int t0 = kt * 32 + 16 * kb2 + 4 * hh, dch = nt * 32 + l31;
        const bf16x8 ah = vs.frag(0, t0, dch), al = vs.frag(1, t0, dch);
        RART_MFMA3(o[nt], ah, al, pbh, pbl)
      }
      if (SCHED_PER_KB2) __builtin_amdgcn_sched_barrier(0);
    }
    if (!SCHED_PER_KB2) __builtin_amdgcn_sched_barrier(0);
  }
  sum += __shfl_xor(sum, 32, 64);
  return 1.0f / sum;
}

// (Round 5: the persistent form of k_vit_attention -- next item's K / V / Q of both planes prefetched into registers -- does not fit here: 112 score
//  registers + 32 output + 64-96 of prefetch exceed the 256 a 7-wave workgroup has (98-132 VGPRs spilled); a split commit -- K after S = K Q^T, V at the
//  item boundary, the next Q into the registers the current Q released -- was written too and spilled 162: the allocator keeps the staged planes and the
//  score registers apart for the whole item.  What is left for this kernel (5 % of a reference-precision ViT-B/16 gradient evaluation) is a prefetch
//  through LDS, i.e. K / V tiles small enough for two buffers: the walking kernel below.)
#ifdef RART_ATT_STAMPS
__device__ unsigned long long g_att_stamps[4096][8][4];       // lab build, per workgroup and wave: [0] staging, [1] Q load + S, [2] soft-max + PV, [3] stores, [4] wave-tiles, [5] workgroups, [6] whole
#define ATT_T(V) const unsigned long long V = __builtin_amdgcn_s_memtime();
#else
#define ATT_T(V)
#endif
// one workgroup per (image, head): K rows and V TRANSPOSED staged through registers (122 KB at 224 tokens: one workgroup per CU)
template <int NKT>
__global__ __launch_bounds__(kAttBlock, 1) void k_vit_attention_pair(const uint16_t* __restrict__ qkv_h, const uint16_t* __restrict__ qkv_l,
                                                                  uint16_t* __restrict__ att_h, uint16_t* __restrict__ att_l, int T, int H,
                                                                  int ld, int D, float scale_log2e) {
  constexpr int TP = NKT * 32, LDV = TP + 4;     // 228-element rows: conflict-free 8-byte reads across 32 lanes
  static_assert(NKT <= PATT_MAX_TILES, "one query tile per wave");
  __shared__ __attribute__((aligned(16))) uint16_t sK[2][TP * PATT_LDK];
  __shared__ __attribute__((aligned(16))) uint16_t sVt[2][PATT_HD * LDV];
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, l31 = lane & 31;
  const size_t boff = (size_t)b * T * ld + h * PATT_HD;
  const uint16_t* const base[2] = {qkv_h + boff, qkv_l + boff};
  ATT_T(t_a)
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    patt_load_rows(sK[p], base[p] + D, T, TP, ld, tid);
    // V transposed: a thread takes 8 channels of FOUR consecutive tokens and writes eight 8-byte runs (one per channel)
    for (int i = tid; i < (TP / 4) * 8; i += kAttBlock) {
      const int tq = i % (TP / 4), c = i / (TP / 4);
      uint32_t w[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        uint4 vv = make_uint4(0, 0, 0, 0);
        if (tq * 4 + u < T) vv = *reinterpret_cast<const uint4*>(base[p] + (size_t)(tq * 4 + u) * ld + 2 * D + c * 8);
        w[u][0] = vv.x; w[u][1] = vv.y; w[u][2] = vv.z; w[u][3] = vv.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint16_t* row = &sVt[p][(c * 8 + 2 * j) * LDV + tq * 4];
        *reinterpret_cast<uint2*>(row) = make_uint2(__builtin_amdgcn_perm(w[1][j], w[0][j], 0x05040100u),
                                                    __builtin_amdgcn_perm(w[3][j], w[2][j], 0x05040100u));
        *reinterpret_cast<uint2*>(row + LDV) = make_uint2(__builtin_amdgcn_perm(w[1][j], w[0][j], 0x07060302u),
                                                          __builtin_amdgcn_perm(w[3][j], w[2][j], 0x07060302u));
      }
    }
  }
  __syncthreads();
  ATT_T(t_b)
  const PattVTransposed<LDV> vs = {{sVt[0], sVt[1]}};
  if (wave < NKT) {                                     // one query tile per wave (at most seven tiles, eight waves)
    ATT_T(t_c)
    const int q = wave * 32 + l31;
    bf16x8 bqh[4], bql[4];
    patt_load_frags(bqh, bql, base[0], base[1], (size_t)q * ld, q < T, hh);
    f32x16 sacc[NKT], o[2];
    patt_scores<NKT, false>(sacc, sK[0], sK[1], bqh, bql);
    ATT_T(t_d)
    const float inv = patt_softmax_pv<NKT, false>(sacc, o, vs, T, scale_log2e);
    ATT_T(t_e)
    if (q < T) {
      const size_t ro = ((size_t)b * T + q) * D + h * PATT_HD;
      patt_store_row<true>(o, inv, att_h + ro, att_l + ro, hh);
    }
#ifdef RART_ATT_STAMPS
    __builtin_amdgcn_s_waitcnt(0);
    ATT_T(t_f)
    if (lane == 0 && blockIdx.x < 4096) {
      unsigned long long* o = g_att_stamps[blockIdx.x][wave];
      o[0] = t_b - t_a; o[1] = t_d - t_c; o[2] = t_e - t_d; o[3] = t_f - t_e;
    }
#endif
  }
}

// ---- the forward again, WALKING (round 6): one workgroup per CU takes a run of (image, head) items; K and V of the NEXT item arrive while the
//      current one computes.  The phase stamps of k_vit_attention_pair (scratch/r6/att_stamps.py) put 45 % of a workgroup's time in the K / V
//      staging, with nothing running beside it: 16 k of 35 k cycles.  Here wave 7 -- the one without a query tile at 197 tokens -- is the loader:
//      both operands go to LDS ROW-MAJOR ([token][72], the K image of the kernel above) with buffer_load ... lds (rart_lds_dma.h), K of item i + 1 during
//      soft-max + P V of item i, V of item i + 1 during S = K Q^T of item i + 1, two barriers per item.  V is no longer transposed on the
//      way in (PattVRowMajor).  Same products in the same order as k_vit_attention_pair: bit-identical output.  Taken for seven key tiles
//      (193 .. 224 tokens) and at least four items per CU.
template <int NKT>
__global__ __launch_bounds__(kAttBlock, 1) void k_vit_attention_pair_walk(const uint16_t* __restrict__ qkv_h, const uint16_t* __restrict__ qkv_l,
                                                                       uint16_t* __restrict__ att_h, uint16_t* __restrict__ att_l, int T, int H,
                                                                       int ld, int D, float scale_log2e, int n_items) {
  constexpr int TP = NKT * 32;
  constexpr int NI = (TP * 9 + 63) / 64;                   // DMA instructions per plane (1 KiB of the padded image each)
  constexpr int PLANE = NI * 1024 / 2;                     // elements per plane buffer (the last instruction's tail included)
  static_assert(NKT <= PATT_MAX_TILES, "wave 7 is the loader");
  __shared__ __attribute__((aligned(16))) uint16_t sK[2][PLANE];
  __shared__ __attribute__((aligned(16))) uint16_t sV[2][PLANE];
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // items blockIdx.x, blockIdx.x + gridDim.x, ...: at any moment neighbouring workgroups hold the heads of ONE image (the 128-byte pieces of a
  // token row they read lie in one DRAM page), as the dispatch order of the one-item kernel had it
  const int first = blockIdx.x, last = n_items, step = gridDim.x;
  if (first >= last) return;
  if (wave == 7) {
    // ---- the loader wave: K and V of the first item, then per item K of the next one during phase 2 and its V during the next phase 1
    const uint32_t k_lds = PATT_LDS_ADDR(sK[0][0]), v_lds = PATT_LDS_ADDR(sV[0][0]);
    const rart_srd_t srd_h = rart_dma_srd(qkv_h), srd_l = rart_dma_srd(qkv_l);
    // one image (column COL of item IT's block) = NI DMA instructions per plane: lane -> 16-byte chunk c of the padded image, token c / 9,
    // chunk c % 9, the ninth chunk and the tokens past T zero-filled by the range check; the per-lane offsets are item-invariant (the loader
    // wave has nothing else to do: they are formed on the fly), the item moves the scalar offset.  Non-temporal: no other workgroup reads
    // K / V of an item (203 -> 199 us per launch)
#define PATT_AW_LOAD(LDS_, IT, COL)                                                                              \
    {                                                                                                            \
      const uint32_t so_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(patt_item_base(IT, H, T, ld) * 2) + (uint32_t)((COL)*2))); \
      _Pragma("unroll") for (int i = 0; i < NI; ++i) {                                                          \
        const int c_ = 64 * i + lane, t_ = c_ / 9, cc_ = c_ - 9 * t_;                                            \
        const uint32_t vo_ = (cc_ < 8 && t_ < T) ? (uint32_t)((t_ * ld + cc_ * 8) * 2) : RART_DMA_OOR;           \
        rart_dma_load16_nt(vo_, srd_h, so_, (LDS_) + i * 1024);                                                  \
        rart_dma_load16_nt(vo_, srd_l, so_, (LDS_) + PLANE * 2 + i * 1024);                                      \
      }                                                                                                          \
    }
    PATT_AW_LOAD(k_lds, first, D)
    PATT_AW_LOAD(v_lds, first, 2 * D)
    rart_dma_wait<0>();
    patt_barrier();
    for (int it = first; it < last; it += step) {
      const bool more = it + step < last;
      rart_dma_wait<0>();                               // V of this item
      patt_barrier();                                   // (B1) every wave is done with K; V is visible
      if (more) PATT_AW_LOAD(k_lds, it + step, D)
      rart_dma_wait<0>();                               // K of the next item
      patt_barrier();                                   // (B2) every wave is done with V; the next K is visible
      if (more) PATT_AW_LOAD(v_lds, it + step, 2 * D)
    }
#undef PATT_AW_LOAD
    return;
  }
  patt_barrier();
  const bool tile = wave < NKT;
  const int q = wave * 32 + l31;
  const PattVRowMajor vs = {{sV[0], sV[1]}};
  for (int it = first; it < last; it += step) {
    bf16x8 bqh[4], bql[4];                              // the wave's Q fragments of this item
    if (tile) patt_load_frags(bqh, bql, qkv_h, qkv_l, patt_item_base(it, H, T, ld) + (size_t)q * ld, q < T, hh);
    // ---- phase 1: S^T = K Q^T
    f32x16 sacc[NKT], o[2];
    if (tile) patt_scores<NKT, false>(sacc, sK[0], sK[1], bqh, bql);
    patt_barrier();                                     // (B1)
    // ---- phase 2: soft-max + O^T = V^T P^T + stores
    if (tile) {
      const float inv = patt_softmax_pv<NKT, true>(sacc, o, vs, T, scale_log2e);
      if (q < T) {
        const size_t ro = ((size_t)(it / H) * T + q) * D + (it % H) * PATT_HD;
        patt_store_row<true>(o, inv, att_h + ro, att_l + ro, hh);
      }
    }
    patt_barrier();                                     // (B2)
  }
}

// ---- fused attention BACKWARD on pairs: two kernels, one workgroup per (image, head) each (or walking, below) ----------------------------
// dQ, dK, dV of softmax(Q K^T / sqrt(d)) V from the Q, K, V, O (the forward's output) and dO pairs.  The bf16 kernel (k_vit_attention_bwd,
// csrc/vit_aux.hip) keeps Q, K, V, dO and two transposed copies in 158 KB of LDS; as pairs that is twice what a CU has, so the two phases
// of that kernel are two launches here, each with HALF of the operands resident (129 KB):
//   k_vit_attention_bwd_q_pair  (a wave owns 32 QUERIES; K, V pairs resident): S^T = K Q^T and dP^T = V dO^T land with lane = query, so max,
//       1 / sum and delta = rowsum(dO * O) need one shuffle; dS (fp32, split into hi + lo) feeds straight back as the B operand of
//       dQ^T = K^T dS^T, whose A operand K^T is gathered from the row-major K image with 2-byte reads in the accumulator's key order (a
//       transposed copy would not fit); writes dQ and the per-query statistics (max, 1 / sum, delta);
//   k_vit_attention_bwd_kv_pair (a wave owns 32 KEYS; Q, dO pairs resident): S = Q K^T and dP = dO V^T are recomputed with lane = key
//       (statistics from LDS), P and dS are the B operands of dV^T = dO^T P and dK^T = Q^T dS (A operands gathered from the row-major Q / dO
//       images), accumulated in registers over the query tiles; writes dK and dV.
// Every contraction is three MFMA products; the soft-max and its derivative are evaluated in fp32 registers.  Replaces, per layer, the
// decomposition into five batched pair products with fp32 score-sized temporaries, two soft-max row kernels and ten transposes.

// Backward-q of the wave's query tile qt: dQ rows and the statistics rows of its 32 queries.  sK / sV: the K and V images of both planes;
// qb / ob / db: the item's qkv, O and dO blocks; dqh / dql + boff: the item's block of the dqkv planes; stat + item * TP: its statistics
// rows (offsets, not advanced pointers: the register allocation of the NKT = 7 kernels follows the form of these addresses).
// WALK: the walking kernel's barriers, where its loader wave hands over or takes back rows of the images -- A6 in front of the last key
// tile of S (the last rows of K have landed), S1 / S3 / S5 after key tiles 1 / 3 / 5 of phase B (a 64-row slice of K and of V is free).
template <int NKT, bool WALK>
__device__ __forceinline__ void patt_bwd_q_tile(int qt, const uint16_t* const (&sK)[2], const uint16_t* const (&sV)[2],
                                                const uint16_t* const (&qb)[2], const uint16_t* const (&ob)[2],
                                                const uint16_t* const (&db)[2], uint16_t* dqh, uint16_t* dql, size_t boff, float4* stat,
                                                size_t item, int T, int ld, int D, float scale, float scale_log2e) {
  const int lane = threadIdx.x & 63, hh = lane >> 5, l31 = lane & 31;
  const int q = qt * 32 + l31;
  bf16x8 bq[2][4], bdo[2][4];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      uint4 vq = make_uint4(0, 0, 0, 0), vd = make_uint4(0, 0, 0, 0);
      if (q < T) {
        vq = *reinterpret_cast<const uint4*>(qb[p] + (size_t)q * ld + kb * 16 + hh * 8);
        vd = *reinterpret_cast<const uint4*>(db[p] + (size_t)q * D + kb * 16 + hh * 8);
      }
      bq[p][kb] = *reinterpret_cast<bf16x8*>(&vq);
      bdo[p][kb] = *reinterpret_cast<bf16x8*>(&vd);
    }
  // delta_q = sum_d dO[q][d] O[q][d]: a lane sums its half of the channels, one shuffle adds the halves
  float delta = 0.f;
  if (q < T) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float ov[8], dv[8];
      join8(*reinterpret_cast<const uint4*>(ob[0] + (size_t)q * D + hh * 32 + c * 8), *reinterpret_cast<const uint4*>(ob[1] + (size_t)q * D + hh * 32 + c * 8), ov);
      join8(*reinterpret_cast<const uint4*>(db[0] + (size_t)q * D + hh * 32 + c * 8), *reinterpret_cast<const uint4*>(db[1] + (size_t)q * D + hh * 32 + c * 8), dv);
#pragma unroll
      for (int j = 0; j < 8; ++j) delta = fmaf(ov[j], dv[j], delta);
    }
  }
  delta += __shfl_xor(delta, 32, 64);
  f32x16 sacc[NKT];
  patt_scores<NKT, WALK>(sacc, sK[0], sK[1], bq[0], bq[1]);
  float m = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if ((NKT - 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh >= T) sacc[NKT - 1][r] = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, sacc[kt][r]);
  m = fmaxf(m, __shfl_xor(m, 32, 64)) * scale_log2e;
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = __builtin_amdgcn_exp2f(fmaf(sacc[kt][r], scale_log2e, -m));
      sacc[kt][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
  if (hh == 0) stat[item * (NKT * 32) + q] = make_float4(m, inv, delta, 0.f);
  const float sinv = scale * inv;
  f32x16 dq[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[nt][r] = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    f32x16 dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const bf16x8 ah = patt_row_frag(sV[0], kt * 32 + l31, kb, hh), al = patt_row_frag(sV[1], kt * 32 + l31, kb, hh);
      RART_MFMA3(dp, ah, al, bdo[0][kb], bdo[1][kb])
    }
#pragma unroll
    for (int kb2 = 0; kb2 < 2; ++kb2) {
      float dsv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) dsv[j] = sinv * sacc[kt][8 * kb2 + j] * (dp[8 * kb2 + j] - delta);
      bf16x8 dsh, dsl;
      patt_split8(dsv, dsh, dsl);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int t0 = kt * 32 + 16 * kb2 + 4 * hh, dch = nt * 32 + l31;
        const bf16x8 ah = patt_tr_frag(sK[0], t0, dch), al = patt_tr_frag(sK[1], t0, dch);
        RART_MFMA3(dq[nt], ah, al, dsh, dsl)
      }
    }
    __builtin_amdgcn_sched_barrier(0);     // one key tile at a time
    if (WALK && (kt == 1 || kt == 3 || kt == 5)) patt_barrier();      // (S1 / S3 / S5)
  }
  // dq[nt][r] = dQ[query q][d = nt*32 + (r&3) + 8*(r>>2) + 4*hh]
  if (q < T) patt_store_row<false>(dq, 1.f, dqh + (boff + (size_t)q * ld), dql + (boff + (size_t)q * ld), hh);
}

template <int NKT>
__global__ __launch_bounds__(kAttBlock, 1) void k_vit_attention_bwd_q_pair(const uint16_t* __restrict__ qkv_h, const uint16_t* __restrict__ qkv_l,
                                                                        const uint16_t* __restrict__ o_h, const uint16_t* __restrict__ o_l,
                                                                        const uint16_t* __restrict__ do_h, const uint16_t* __restrict__ do_l,
                                                                        uint16_t* __restrict__ dq_h, uint16_t* __restrict__ dq_l,
                                                                        float4* __restrict__ stats, int T, int H, int ld, int D, float scale,
                                                                        float scale_log2e) {
  constexpr int TP = NKT * 32;
  static_assert(NKT <= PATT_MAX_TILES, "one query tile per wave");
  __shared__ __attribute__((aligned(16))) uint16_t sK[2][TP * PATT_LDK];
  __shared__ __attribute__((aligned(16))) uint16_t sV[2][TP * PATT_LDK];
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int tid = threadIdx.x, wave = tid >> 6;
  const size_t boff = (size_t)b * T * ld + h * PATT_HD, doff = (size_t)b * T * D + h * PATT_HD;
  const uint16_t* const qb[2] = {qkv_h + boff, qkv_l + boff};
  const uint16_t* const ob[2] = {o_h + doff, o_l + doff};
  const uint16_t* const db[2] = {do_h + doff, do_l + doff};
  const uint16_t* const pK[2] = {sK[0], sK[1]};
  const uint16_t* const pV[2] = {sV[0], sV[1]};
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    patt_load_rows(sK[p], qb[p] + D, T, TP, ld, tid);
    patt_load_rows(sV[p], qb[p] + 2 * D, T, TP, ld, tid);
  }
  __syncthreads();
  if (wave < NKT)                                       // one query tile per wave (at most seven tiles, eight waves)
    patt_bwd_q_tile<NKT, false>(wave, pK, pV, qb, ob, db, dq_h, dq_l, boff, stats, (size_t)blockIdx.x, T, ld, D, scale, scale_log2e);
}

// The backward-q, WALKING.  Phase B (dP, dS, dQ) walks the key tiles in order, every wave the same, and is the LAST reader of a key tile's
// K and V rows: once all waves are past key tiles 2k, 2k + 1 (barriers S1 / S3 / S5) the loader wave sends the NEXT item's 64-row slice
// of K and of V there (nine DMA instructions per image).  The last slice (rows 192 ..) follows the item boundary: K's is needed by the
// seventh key tile of S = K Q^T (barrier A6 in front of it), V's not before phase B.
template <int NKT>
__global__ __launch_bounds__(kAttBlock, 1) void k_vit_attention_bwd_q_pair_walk(const uint16_t* __restrict__ qkv_h, const uint16_t* __restrict__ qkv_l,
                                                                        const uint16_t* __restrict__ o_h, const uint16_t* __restrict__ o_l,
                                                                        const uint16_t* __restrict__ do_h, const uint16_t* __restrict__ do_l,
                                                                        uint16_t* __restrict__ dq_h, uint16_t* __restrict__ dq_l,
                                                                        float4* __restrict__ stats, int T, int H, int ld, int D, float scale,
                                                                        float scale_log2e, int n_items) {
  constexpr int TP = NKT * 32;
  constexpr int NI = (TP * 9 + 63) / 64;                   // DMA instructions per plane of a padded [token][72] image
  constexpr int PLANE = NI * 512;                          // elements per plane buffer (the last instruction's tail included)
  static_assert(NKT == 7, "wave 7 is the loader: one query tile per compute wave");
  __shared__ __attribute__((aligned(16))) uint16_t sK[2][PLANE];
  __shared__ __attribute__((aligned(16))) uint16_t sV[2][PLANE];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int first = blockIdx.x, step = gridDim.x;          // items first, first + step, ...: neighbouring workgroups hold the heads of one image
  if (first >= n_items) return;
  if (wave == 7) {
    // ---- the loader wave
    const uint32_t k_lds = PATT_LDS_ADDR(sK[0][0]), v_lds = PATT_LDS_ADDR(sV[0][0]);
    const rart_srd_t srd_h = rart_dma_srd(qkv_h), srd_l = rart_dma_srd(qkv_l);
    // DMA instructions I0 .. I1 - 1 of item IT's K and V images (the forward's chunk arithmetic; nine instructions = 64 rows)
#define PATT_BQ_SLICE(IT, I0, I1)                                                                                \
    {                                                                                                            \
      const uint32_t ib_ = (uint32_t)(patt_item_base(IT, H, T, ld) * 2);                                         \
      const uint32_t ko_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ib_ + (uint32_t)(D * 2)));             \
      const uint32_t vo2_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ib_ + (uint32_t)(D * 4)));            \
      _Pragma("unroll") for (int i = (I0); i < (I1); ++i) {                                                     \
        const int c_ = 64 * i + lane, t_ = c_ / 9, cc_ = c_ - 9 * t_;                                            \
        const uint32_t vo_ = (cc_ < 8 && t_ < T) ? (uint32_t)((t_ * ld + cc_ * 8) * 2) : RART_DMA_OOR;           \
        rart_dma_load16_nt(vo_, srd_h, ko_, k_lds + i * 1024);                                                   \
        rart_dma_load16_nt(vo_, srd_l, ko_, k_lds + PLANE * 2 + i * 1024);                                       \
        rart_dma_load16_nt(vo_, srd_h, vo2_, v_lds + i * 1024);                                                  \
        rart_dma_load16_nt(vo_, srd_l, vo2_, v_lds + PLANE * 2 + i * 1024);                                      \
      }                                                                                                          \
    }
    PATT_BQ_SLICE(first, 0, 27)
    for (int it = first; it < n_items; it += step) {
      const bool more = it + step < n_items;
      rart_dma_wait<0>();                               // rows 0 .. 191 of this item's K and V
      patt_barrier();                                   // (E) the item starts
      PATT_BQ_SLICE(it, 27, NI)                         // rows 192 ..: free since the previous item's last key tile
      rart_dma_wait<0>();
      patt_barrier();                                   // (A6) in front of the seventh key tile of S = K Q^T
      patt_barrier();                                   // (S1) phase B is past key tiles 0, 1
      if (more) PATT_BQ_SLICE(it + step, 0, 9)
      patt_barrier();                                   // (S3)
      if (more) PATT_BQ_SLICE(it + step, 9, 18)
      patt_barrier();                                   // (S5)
      if (more) PATT_BQ_SLICE(it + step, 18, 27)
    }
#undef PATT_BQ_SLICE
    rart_dma_wait<0>();
    return;
  }
  const uint16_t* const pK[2] = {sK[0], sK[1]};
  const uint16_t* const pV[2] = {sV[0], sV[1]};
  for (int it = first; it < n_items; it += step) {
    const size_t boff = patt_item_base(it, H, T, ld), doff = patt_item_base(it, H, T, D);
    const uint16_t* const qb[2] = {qkv_h + boff, qkv_l + boff};
    const uint16_t* const ob[2] = {o_h + doff, o_l + doff};
    const uint16_t* const db[2] = {do_h + doff, do_l + doff};
    patt_barrier();                                     // (E)
    patt_bwd_q_tile<NKT, true>(wave, pK, pV, qb, ob, db, dq_h, dq_l, boff, stats, (size_t)it, T, ld, D, scale, scale_log2e);
  }
}

// Backward-kv of the wave's key tile kt: the dK and dV rows of its 32 keys, accumulated over the query tiles.  sQ / sdO: the Q and dO
// images of both planes; sStat: the item's statistics in LDS; qb: the item's qkv block (K and V fragments come from global memory);
// dqh / dql + boff: the item's block of the dqkv planes.  WALK: the walking kernel's barriers S1 / S3 / S5 after query tiles 1 / 3 / 5 -- a
// 64-row slice of Q and dO is free for the loader wave.
template <int NKT, bool WALK>
__device__ __forceinline__ void patt_bwd_kv_tile(int kt, const uint16_t* const (&sQ)[2], const uint16_t* const (&sdO)[2], const float4* sStat,
                                                 const uint16_t* const (&qb)[2], uint16_t* dqh, uint16_t* dql, size_t boff, int T, int ld, int D,
                                                 float scale, float scale_log2e) {
  const int lane = threadIdx.x & 63, hh = lane >> 5, l31 = lane & 31;
  const int key = kt * 32 + l31;
  const bool key_ok = key < T;
  bf16x8 bk[2][4], bv[2][4];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      uint4 vk = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
      if (key_ok) {
        vk = *reinterpret_cast<const uint4*>(qb[p] + (size_t)key * ld + D + kb * 16 + hh * 8);
        vv = *reinterpret_cast<const uint4*>(qb[p] + (size_t)key * ld + 2 * D + kb * 16 + hh * 8);
      }
      bk[p][kb] = *reinterpret_cast<bf16x8*>(&vk);
      bv[p][kb] = *reinterpret_cast<bf16x8*>(&vv);
    }
  // dV^T = dO^T . P and dK^T = Q^T . dS (operands swapped): lane = key, registers = channels
  f32x16 dvv[2], dkk[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dvv[nt][r] = dkk[nt][r] = 0.f;
#pragma unroll 1
  for (int qt = 0; qt < NKT; ++qt) {
    f32x16 sa, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) sa[r] = dp[r] = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const bf16x8 qh = patt_row_frag(sQ[0], qt * 32 + l31, kb, hh), ql = patt_row_frag(sQ[1], qt * 32 + l31, kb, hh);
      const bf16x8 dh = patt_row_frag(sdO[0], qt * 32 + l31, kb, hh), dl = patt_row_frag(sdO[1], qt * 32 + l31, kb, hh);
      RART_MFMA3(sa, qh, ql, bk[0][kb], bk[1][kb])
      RART_MFMA3(dp, dh, dl, bv[0][kb], bv[1][kb])
    }
    // lane = key kt*32 + l31; register r = query qt*32 + (r&3) + 8*(r>>2) + 4*hh (queries past the sequence have zero Q / dO rows:
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
      bf16x8 pbh, pbl, dbh, dbl;
      patt_split8(pw, pbh, pbl);
      patt_split8(dw, dbh, dbl);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int t0 = qt * 32 + 16 * kb2 + 4 * hh, dch = nt * 32 + l31;
        const bf16x8 oh = patt_tr_frag(sdO[0], t0, dch), ol = patt_tr_frag(sdO[1], t0, dch);
        const bf16x8 qh = patt_tr_frag(sQ[0], t0, dch), ql = patt_tr_frag(sQ[1], t0, dch);
        RART_MFMA3(dvv[nt], oh, ol, pbh, pbl)
        RART_MFMA3(dkk[nt], qh, ql, dbh, dbl)
      }
    }
    if (WALK && (qt == 1 || qt == 3 || qt == 5)) patt_barrier();       // (S1 / S3 / S5)
  }
  // dkk / dvv[nt][r] = dK / dV[key][d = nt*32 + (r&3) + 8*(r>>2) + 4*hh]: 8-byte runs of the lane's own key row
  if (key_ok) {
    const size_t ro = boff + (size_t)key * ld;
    patt_store_row<false>(dkk, 1.f, dqh + ro + D, dql + ro + D, hh);
    patt_store_row<false>(dvv, 1.f, dqh + ro + 2 * D, dql + ro + 2 * D, hh);
  }
}

template <int NKT>
__global__ __launch_bounds__(kAttBlock, 1) void k_vit_attention_bwd_kv_pair(const uint16_t* __restrict__ qkv_h, const uint16_t* __restrict__ qkv_l,
                                                                         const uint16_t* __restrict__ do_h, const uint16_t* __restrict__ do_l,
                                                                         uint16_t* __restrict__ dq_h, uint16_t* __restrict__ dq_l,
                                                                         const float4* __restrict__ stats, int T, int H, int ld, int D, float scale,
                                                                         float scale_log2e) {
  constexpr int TP = NKT * 32;
  static_assert(NKT <= PATT_MAX_TILES, "one key tile per wave");
  __shared__ __attribute__((aligned(16))) uint16_t sQ[2][TP * PATT_LDK];
  __shared__ __attribute__((aligned(16))) uint16_t sdO[2][TP * PATT_LDK];
  __shared__ __attribute__((aligned(16))) float4 sStat[TP];
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int tid = threadIdx.x, wave = tid >> 6;
  const size_t boff = (size_t)b * T * ld + h * PATT_HD, doff = (size_t)b * T * D + h * PATT_HD;
  const uint16_t* const qb[2] = {qkv_h + boff, qkv_l + boff};
  const uint16_t* const db[2] = {do_h + doff, do_l + doff};
  const uint16_t* const pQ[2] = {sQ[0], sQ[1]};
  const uint16_t* const pdO[2] = {sdO[0], sdO[1]};
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    patt_load_rows(sQ[p], qb[p], T, TP, ld, tid);
    patt_load_rows(sdO[p], db[p], T, TP, D, tid);
  }
  for (int i = tid; i < TP; i += kAttBlock) sStat[i] = stats[(size_t)blockIdx.x * TP + i];
  __syncthreads();
  if (wave < NKT)                                       // one key tile per wave (at most seven tiles, eight waves)
    patt_bwd_kv_tile<NKT, false>(wave, pQ, pdO, sStat, qb, dq_h, dq_l, boff, T, ld, D, scale, scale_log2e);
}

// The backward-kv, WALKING.  The compute waves consume Q and dO one 32-query tile at a time, in the same order, so the rows of a 64-row
// slice are free once every wave is past its two tiles (barriers S1 / S3 / S5): the loader wave sends the NEXT item's slice there while
// the current item still works on the later ones; the last slice (rows 192 ..) follows the item boundary and has until tile 6.  The
// statistics of the next item go to the other half of sStat2.
template <int NKT>
__global__ __launch_bounds__(kAttBlock, 1) void k_vit_attention_bwd_kv_pair_walk(const uint16_t* __restrict__ qkv_h, const uint16_t* __restrict__ qkv_l,
                                                                         const uint16_t* __restrict__ do_h, const uint16_t* __restrict__ do_l,
                                                                         uint16_t* __restrict__ dq_h, uint16_t* __restrict__ dq_l,
                                                                         const float4* __restrict__ stats, int T, int H, int ld, int D, float scale,
                                                                         float scale_log2e, int n_items) {
  constexpr int TP = NKT * 32;
  constexpr int NI = (TP * 9 + 63) / 64;                   // DMA instructions per plane of a padded [token][72] image
  constexpr int PLANE = NI * 512;                          // elements per plane buffer
  static_assert(NKT == 7 && NI == 32, "wave 7 is the loader; slices of 64 rows = 9 instructions, the last one 5");
  __shared__ __attribute__((aligned(16))) uint16_t sQ[2][PLANE];
  __shared__ __attribute__((aligned(16))) uint16_t sdO[2][PLANE];
  __shared__ __attribute__((aligned(16))) float4 sStat2[2][TP];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int first = blockIdx.x, step = gridDim.x;
  if (first >= n_items) return;
  if (wave == 7) {
    // ---- the loader wave
    const uint32_t q_lds = PATT_LDS_ADDR(sQ[0][0]), d_lds = PATT_LDS_ADDR(sdO[0][0]);
    const rart_srd_t sq_h = rart_dma_srd(qkv_h), sq_l = rart_dma_srd(qkv_l), sd_h = rart_dma_srd(do_h), sd_l = rart_dma_srd(do_l);
    // DMA instructions I0 .. I1 - 1 of item IT's Q and dO images (the forward's chunk arithmetic; the two operands have their own row strides)
#define PATT_BK_SLICE(IT, I0, I1)                                                                                \
    {                                                                                                            \
      const uint32_t qo_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)(patt_item_base(IT, H, T, ld) * 2));    \
      const uint32_t do_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)(patt_item_base(IT, H, T, D) * 2));     \
      _Pragma("unroll") for (int i = (I0); i < (I1); ++i) {                                                     \
        const int c_ = 64 * i + lane, t_ = c_ / 9, cc_ = c_ - 9 * t_;                                            \
        const bool ok_ = cc_ < 8 && t_ < T;                                                                      \
        const uint32_t vq_ = ok_ ? (uint32_t)((t_ * ld + cc_ * 8) * 2) : RART_DMA_OOR;                           \
        const uint32_t vd_ = ok_ ? (uint32_t)((t_ * D + cc_ * 8) * 2) : RART_DMA_OOR;                            \
        rart_dma_load16_nt(vq_, sq_h, qo_, q_lds + i * 1024);                                                    \
        rart_dma_load16_nt(vq_, sq_l, qo_, q_lds + PLANE * 2 + i * 1024);                                        \
        rart_dma_load16_nt(vd_, sd_h, do_, d_lds + i * 1024);                                                    \
        rart_dma_load16_nt(vd_, sd_l, do_, d_lds + PLANE * 2 + i * 1024);                                        \
      }                                                                                                          \
    }
#define PATT_BK_STATS(IT, PAR)                                     \
    for (int i = lane; i < TP; i += 64) sStat2[PAR][i] = stats[(size_t)(IT)*TP + i];
    PATT_BK_SLICE(first, 0, 27)
    PATT_BK_STATS(first, 0)
    int par = 0;
    for (int it = first; it < n_items; it += step) {
      const bool more = it + step < n_items;
      rart_dma_wait<0>();                               // rows 0 .. 191 of this item (and its statistics) are in LDS
      patt_barrier();                                   // (E) the item starts
      PATT_BK_SLICE(it, 27, 32)                         // rows 192 ..: free since the previous item's last tile
      if (more) PATT_BK_STATS(it + step, par ^ 1)
      rart_dma_wait<0>();
      patt_barrier();                                   // (S1) tiles 0, 1 done everywhere; the last slice is visible
      if (more) PATT_BK_SLICE(it + step, 0, 9)
      patt_barrier();                                   // (S3)
      if (more) PATT_BK_SLICE(it + step, 9, 18)
      patt_barrier();                                   // (S5)
      if (more) PATT_BK_SLICE(it + step, 18, 27)
      par ^= 1;
    }
#undef PATT_BK_STATS
#undef PATT_BK_SLICE
    rart_dma_wait<0>();
    return;
  }
  const uint16_t* const pQ[2] = {sQ[0], sQ[1]};
  const uint16_t* const pdO[2] = {sdO[0], sdO[1]};
  int par = 0;
  for (int it = first; it < n_items; it += step) {
    const size_t boff = patt_item_base(it, H, T, ld);
    const uint16_t* const qb[2] = {qkv_h + boff, qkv_l + boff};
    patt_barrier();                                     // (E)
    patt_bwd_kv_tile<NKT, true>(wave, pQ, pdO, sStat2[par], qb, dq_h, dq_l, boff, T, ld, D, scale, scale_log2e);
    par ^= 1;
  }
}
#undef PATT_LDS_ADDR
#undef RART_MFMA3


// The walking decision of both attention entries: the number of workgroups to launch, one per CU, or 0 for the one-item kernels.  The
// walking kernels exist for seven key tiles (wave 7 is free to load), pay off from four items per CU, and address a qkv plane with 32-bit
// DMA offsets (dO is a third of that).  RART_ATT_WALK=0 selects the one-item kernels; it is read at every call (the tests flip it).
int patt_walk_cus(int n, int tokens, int heads, int D) {
  const char* we = getenv("RART_ATT_WALK");
  if (we && atoi(we) == 0) return 0;
  if ((tokens + 31) / 32 != 7 || (long long)n * tokens * 3 * D * 2 >= (1ll << 31)) return 0;
  static int cu_cache[64] = {0};                     // compute units per device
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (cu_cache[dev] == 0 && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) cu_cache[dev] = cus;
  cus = cu_cache[dev];
  return cus > 0 && (long long)n * heads >= 4ll * cus ? cus : 0;
}
}  // namespace

extern "C" {

int rart_softmax_rows_pair(const float* scores, void* probs_hi, void* probs_lo, int64_t rows, int n_valid, int ld_in, int ld_out,
                           float scale, rart_stream_t stream) {
  RART_CHECK_ARG(scores && probs_hi && probs_lo && rows > 0 && n_valid > 0 && ld_in >= n_valid && ld_out >= n_valid,
                 "rart_softmax_rows_pair: bad arguments");
  RART_CHECK_ARG(ld_in % 4 == 0 && ld_out % 4 == 0 && ld_in <= 256 && ld_out <= 256,
                 "rart_softmax_rows_pair: leading dimensions must be multiples of 4, at most 256");
  hipLaunchKernelGGL(k_softmax_rows_pair, dim3((uint32_t)((rows + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0,
                     (hipStream_t)stream, scores, (uint16_t*)probs_hi, (uint16_t*)probs_lo, (long long)rows, n_valid, ld_in, ld_out, scale);
  RART_CHECK_LAUNCH("rart_softmax_rows_pair");
  return RART_OK;
}

int rart_softmax_bwd_rows_pair(const void* probs_hi, const void* probs_lo, const float* dprobs, void* ds_hi, void* ds_lo, int64_t rows,
                               int n_valid, int ld_p, int ld_dp, int ld_out, float scale, rart_stream_t stream) {
  RART_CHECK_ARG(probs_hi && probs_lo && dprobs && ds_hi && ds_lo && rows > 0 && n_valid > 0 && ld_p >= n_valid && ld_dp >= n_valid &&
                     ld_out >= n_valid, "rart_softmax_bwd_rows_pair: bad arguments");
  RART_CHECK_ARG(ld_p % 4 == 0 && ld_dp % 4 == 0 && ld_out % 4 == 0 && ld_p <= 256 && ld_dp <= 256 && ld_out <= 256,
                 "rart_softmax_bwd_rows_pair: leading dimensions must be multiples of 4, at most 256");
  hipLaunchKernelGGL(k_softmax_bwd_rows_pair, dim3((uint32_t)((rows + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0,
                     (hipStream_t)stream, (const uint16_t*)probs_hi, (const uint16_t*)probs_lo, dprobs, (uint16_t*)ds_hi, (uint16_t*)ds_lo,
                     (long long)rows, n_valid, ld_p, ld_dp, ld_out, scale);
  RART_CHECK_LAUNCH("rart_softmax_bwd_rows_pair");
  return RART_OK;
}

int rart_vit_attention_pair(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, int n, int tokens, int heads, int head_dim,
                            rart_stream_t stream) {
  RART_CHECK_ARG(qkv_hi && qkv_lo && out_hi && out_lo && n > 0 && tokens > 0 && heads > 0, "rart_vit_attention_pair: bad arguments");
  RART_CHECK_ARG(head_dim == 64, "rart_vit_attention_pair: head_dim must be 64 (ViT-B/16)");
  RART_CHECK_ARG(tokens <= 224, "rart_vit_attention_pair: at most 224 tokens (197 for 224x224 / patch 16)");
  const int D = heads * head_dim;
  const float scale_log2e = (1.0f / sqrtf((float)head_dim)) * 1.4426950408889634f;
  const dim3 grid((uint32_t)(n * heads));
  hipStream_t st = (hipStream_t)stream;
  if (const int cus = patt_walk_cus(n, tokens, heads, D)) {
    hipLaunchKernelGGL(k_vit_attention_pair_walk<7>, dim3((uint32_t)cus), dim3(kAttBlock), 0, st, (const uint16_t*)qkv_hi,
                       (const uint16_t*)qkv_lo, (uint16_t*)out_hi, (uint16_t*)out_lo, tokens, heads, 3 * D, D, scale_log2e, n * heads);
    RART_CHECK_LAUNCH("rart_vit_attention_pair (walking)");
    return RART_OK;
  }
#define RART_PATT_CASE(N) case N: hipLaunchKernelGGL(k_vit_attention_pair<N>, grid, dim3(kAttBlock), 0, st, (const uint16_t*)qkv_hi, \
    (const uint16_t*)qkv_lo, (uint16_t*)out_hi, (uint16_t*)out_lo, tokens, heads, 3 * D, D, scale_log2e); break;
  switch ((tokens + 31) / 32) {                   // key tiles: only the last one is partial
    RART_PATT_CASE(1) RART_PATT_CASE(2) RART_PATT_CASE(3) RART_PATT_CASE(4) RART_PATT_CASE(5) RART_PATT_CASE(6)
    default: hipLaunchKernelGGL(k_vit_attention_pair<7>, grid, dim3(kAttBlock), 0, st, (const uint16_t*)qkv_hi, (const uint16_t*)qkv_lo,
                                (uint16_t*)out_hi, (uint16_t*)out_lo, tokens, heads, 3 * D, D, scale_log2e); break;
  }
#undef RART_PATT_CASE
  RART_CHECK_LAUNCH("rart_vit_attention_pair");
  return RART_OK;
}

int rart_vit_attention_bwd_pair(const void* qkv_hi, const void* qkv_lo, const void* out_hi, const void* out_lo, const void* dout_hi,
                                const void* dout_lo, void* dqkv_hi, void* dqkv_lo, float* stats, int n, int tokens, int heads, int head_dim,
                                rart_stream_t stream) {
  RART_CHECK_ARG(qkv_hi && qkv_lo && out_hi && out_lo && dout_hi && dout_lo && dqkv_hi && dqkv_lo && stats && n > 0 && tokens > 0 && heads > 0,
                 "rart_vit_attention_bwd_pair: bad arguments");
  RART_CHECK_ARG(head_dim == 64, "rart_vit_attention_bwd_pair: head_dim must be 64 (ViT-B/16)");
  RART_CHECK_ARG(tokens <= 224, "rart_vit_attention_bwd_pair: at most 224 tokens (197 for 224x224 / patch 16)");
  const int D = heads * head_dim;
  const float scale = 1.0f / sqrtf((float)head_dim), sl2e = scale * 1.4426950408889634f;
  const dim3 grid((uint32_t)(n * heads));
  hipStream_t st = (hipStream_t)stream;
  const uint16_t *qh = (const uint16_t*)qkv_hi, *ql = (const uint16_t*)qkv_lo, *oh = (const uint16_t*)out_hi, *ol = (const uint16_t*)out_lo;
  const uint16_t *dh = (const uint16_t*)dout_hi, *dl = (const uint16_t*)dout_lo;
  uint16_t *gh = (uint16_t*)dqkv_hi, *gl = (uint16_t*)dqkv_lo;
  float4* s4 = (float4*)stats;
  if (const int cus = patt_walk_cus(n, tokens, heads, D)) {
    hipLaunchKernelGGL(k_vit_attention_bwd_q_pair_walk<7>, dim3((uint32_t)cus), dim3(kAttBlock), 0, st, qh, ql, oh, ol, dh, dl, gh, gl, s4, tokens,
                       heads, 3 * D, D, scale, sl2e, n * heads);
    hipLaunchKernelGGL(k_vit_attention_bwd_kv_pair_walk<7>, dim3((uint32_t)cus), dim3(kAttBlock), 0, st, qh, ql, dh, dl, gh, gl,
                       (const float4*)s4, tokens, heads, 3 * D, D, scale, sl2e, n * heads);
    RART_CHECK_LAUNCH("rart_vit_attention_bwd_pair (walking)");
    return RART_OK;
  }
#define RART_PATTB_CASE(N)                                                                                                              \
  hipLaunchKernelGGL(k_vit_attention_bwd_q_pair<N>, grid, dim3(kAttBlock), 0, st, qh, ql, oh, ol, dh, dl, gh, gl, s4, tokens, heads, 3 * D, D, \
                     scale, sl2e);                                                                                                      \
  hipLaunchKernelGGL(k_vit_attention_bwd_kv_pair<N>, grid, dim3(kAttBlock), 0, st, qh, ql, dh, dl, gh, gl, (const float4*)s4, tokens, heads,  \
                     3 * D, D, scale, sl2e);
  switch ((tokens + 31) / 32) {                   // key tiles: only the last one is partial
    case 1: RART_PATTB_CASE(1) break;
    case 2: RART_PATTB_CASE(2) break;
    case 3: RART_PATTB_CASE(3) break;
    case 4: RART_PATTB_CASE(4) break;
    case 5: RART_PATTB_CASE(5) break;
    case 6: RART_PATTB_CASE(6) break;
    default: RART_PATTB_CASE(7) break;
  }
#undef RART_PATTB_CASE
  RART_CHECK_LAUNCH("rart_vit_attention_bwd_pair");
  return RART_OK;
}

}  // extern "C"

#ifdef RART_ATT_STAMPS
extern "C" int rart_debug_att_stamps(unsigned long long* out) {      // lab build only: out[4096][8][4]
  if (hipDeviceSynchronize() != hipSuccess) return RART_ERR_HIP;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_att_stamps), sizeof(unsigned long long) * 4096 * 8 * 4) == hipSuccess ? RART_OK : RART_ERR_HIP;
}
#endif
