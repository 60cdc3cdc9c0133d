// Fused stem BACKWARD of the reference-precision ("fp32x") ResNet-50 engine (gfx950): max-pool backward + ReLU mask + transposed 7x7/2
// convolution to the fp32 image gradient in ONE kernel, every tensor a hi + lo pair of bf16 planes, every contraction the three MFMA
// products lo.hi + hi.lo + hi.hi (fp32 accumulation).
//
// Replaces the chain k_maxpool_bwd_pair -> patches GEMM (k_gemm_pair, N = 152, fp32 out) -> k_stem_col2im_f32, which wrote and re-read the
// 112 x 112 x 64 gradient pair (2 x 411 MB) and a 1.95 GB fp32 patch tensor per 256 images: 2.5 ms of the 21 ms of a gradient evaluation
// (profiles/r04_bench_kernel_stats.csv: 344 + 723 + 1 477 us).  Same structure as k_stem_bwd_fused (csrc/stem_fused.hip, which states the
// math): a workgroup owns 16 x 16 positions of the stem-output grid, rebuilds the 19 x 19 halo tile of the gradient at the stem output in
// LDS from the pooled gradient pair and the argmax codes (code 15 = window maximum <= 0 = ReLU dead), walks the 16 taps as an implicit
// GEMM (M = positions, K = 16 taps x 64 channels, N = 12 = 4 pixel parities x 3 colours) on v_mfma_f32_16x16x32_bf16 and writes a
// 32 x 32 x 3 fp32 tile.  The pair doubles every LDS image, so the K dimension is walked in two channel halves (32 channels = one MFMA K
// step per tap): stage -> pool backward -> weights -> 16 taps, twice, into the same accumulators.  The weight fragments of a half (32 KB)
// go through LDS once per workgroup, in the region the raw pooled tile has left by then: fetched per wave from global memory they were
// 256 KB per tile against 39 KB of pooled gradient and codes, and the texture-address unit they went through paced the kernel.  78 KB of
// LDS, two workgroups per CU whose phases overlap, as in the bf16 kernel.
//
// Reference step: the autograd pass of every attack iteration (RobustART/noise/utils/adv/attack.py:21-22 via foolbox;
// Attacks/autoattack/autopgd_base.py:271-289, fp32) through conv1 / bn1 / relu / maxpool of the public ResNet-50
// (RobustART/model/__init__.py:1 -> absent submodule; robustart_amd/model/resnet_torch.py states it).
#include "rart_common.h"
#include "rart_bf16_helpers.h"

#include <type_traits>

// Lab builds only: -DRART_STEM_STAMPS sums s_memtime intervals per phase and wave into g_sp_stamps ([0] backward: stage, pool backward,
// weights + taps, epilogue, whole kernel, waves; [1] forward: stage, row taps, barrier after them, ReLU + tile store, pool + global store,
// tiles x waves, whole loop, waves), read and reset by rart_debug_stem_stamps, an export of that build alone (profiles/stem_pair_stamps.py).
// A stamp does not wait for outstanding loads or MFMAs.  -DRART_STEM_U8_PREFETCH=1 gives the uint8 forward the fp32 one's source prefetch.
#ifdef RART_STEM_STAMPS
__device__ unsigned long long g_sp_stamps[2][8];
#define SP_T(V) const unsigned long long V = __builtin_amdgcn_s_memtime();
#define SP_ST(...) __VA_ARGS__
#else
#define SP_T(V)
#define SP_ST(...)
#endif
#ifndef RART_STEM_U8_PREFETCH
#define RART_STEM_U8_PREFETCH 0
#endif

namespace {
using namespace rart_bf16;
constexpr int T = 16;                     // positions per tile side
constexpr int HT = T + 3;                 // halo tile side (dp, dq in -1..2)
constexpr int NPOS_PAD = 368;             // 361 rounded up to a multiple of 16: chunk planes start on a 256-byte bank row
constexpr int PT = T / 2 + 3;             // pooled positions per side that reach the halo tile (11)
constexpr int PTS = 12;                   // pooled row stride in LDS: the pool backward walks PTS windows per row, so a window's slot is
                                          // its walk index + a constant and every read below is conflict free
constexpr int NPOOL = PT * PT;            // 121
constexpr int NPOOL_PAD = PT * PTS;       // 132
constexpr int OT = 2 * T;                 // image pixels per tile side (32)
constexpr int OLD = OT + 1;               // padded fp32 output row in LDS
constexpr int OPL = OT * OLD + 3;         // colour plane stride: = 3 mod 32, so the 24 lanes of an epilogue store meet at most two per bank
// (PTS, NPOS_PAD, HT and the lane -> window walks of pool_bwd_class_pair are mirrored in tests/test_stem_pair_bank_model.py, which
// holds the modelled LDS cycles of the reads below at the conflict-free count)
constexpr int DZ_BYTES = 2 * 4 * NPOS_PAD * 16;       // [hi | lo][4 chunks of a channel half][NPOS_PAD] x 16 B
constexpr int DP_BYTES = 2 * NPOOL_PAD * 4 * 16;      // [hi | lo][NPOOL_PAD][4 chunks]
constexpr int ARG_BYTES = NPOOL_PAD * 4 * 8;          // [NPOOL_PAD][4 chunks] x 8 codes
constexpr int W_BYTES = 2 * 16 * 64 * 16;             // the weight fragments of a channel half: [hi | lo][16 taps][64 lanes] x 16 B (32 KB)
constexpr int RW_BYTES = W_BYTES;                     // one region: raw pooled tile, then the half's weights, at the end the output tile
static_assert(DP_BYTES + ARG_BYTES <= RW_BYTES && 3 * OPL * 4 <= RW_BYTES, "raw pooled tile and output tile must fit the weight region");
static_assert(2 * (DZ_BYTES + RW_BYTES) <= 160 * 1024, "two workgroups per CU");

// the halo positions whose stem row has parity EY and whose stem column has parity EX (see pool_bwd_class in stem_fused.hip): one
// window per even coordinate, two per odd; the gradient of a position is the fp32 sum of the pair VALUES of its matching windows
template <int EY, int EX>
__device__ __forceinline__ void pool_bwd_class_pair(uint4* sDz1, const uint4* sDp, const uint2* sArg, int tid, int a0, int b0, int qy0,
                                                    int qx0, int oh, int ow) {
  constexpr int NY = EY ? (HT + 1) / 2 : HT / 2, NX = EX ? (HT + 1) / 2 : HT / 2;
  constexpr int NYS = EY ? 2 : 1, NXS = EX ? 2 : 1;
  // 32 lanes = 8 consecutive windows of the PTS-wide walk x 4 chunks, window in the low bits: a 16-lane group of a 16-byte read then
  // holds four windows with distinct slot mod 4 per chunk, the 32 lanes of an 8-byte read eight consecutive windows
  for (int i = tid; i < ((4 * NY * PTS + 31) & ~31); i += 256) {
    const int c = (i >> 3) & 3, j = (i & 7) + ((i >> 5) << 3);
    const int iy = j / PTS, ix = j - iy * PTS;
    if (iy >= NY || ix >= NX) continue;
    const int hy = 2 * iy + (EY ? 0 : 1), hx = 2 * ix + (EX ? 0 : 1);
    const int py = a0 - 1 + hy, px = b0 - 1 + hx;           // stem-output coordinates
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if ((unsigned)py < (unsigned)oh && (unsigned)px < (unsigned)ow) {
#pragma unroll
      for (int ia = 0; ia < NYS; ++ia) {
        const int qy = (py >> 1) + ia;
        const uint32_t ky = (uint32_t)(py - (2 * qy - 1));
#pragma unroll
        for (int ib = 0; ib < NXS; ++ib) {
          const int qx = (px >> 1) + ib;
          const uint32_t mine = (ky * 3 + (uint32_t)(px - (2 * qx - 1))) * 0x01010101u;
          const int lp = (qy - qy0) * PTS + (qx - qx0);     // out-of-grid windows hold code 15 / zeros
          const uint2 cd = sArg[lp * 4 + c];
          const uint4 dh = sDp[lp * 4 + c], dl = sDp[(NPOOL_PAD + lp) * 4 + c];
          const uint32_t cw[2] = {cd.x, cd.y};
          const uint32_t hw_[4] = {dh.x, dh.y, dh.z, dh.w}, lw_[4] = {dl.x, dl.y, dl.z, dl.w};
#pragma unroll
          for (int hw = 0; hw < 2; ++hw) {
            // codes are < 16, so (code ^ mine) + 0x7F sets bit 7 of a byte exactly when the byte differs
            const uint32_t ne = ((cw[hw] ^ mine) + 0x7F7F7F7Fu) & 0x80808080u;
            const uint32_t eq = (ne ^ 0x80808080u) >> 7;              // 1 per equal byte
            const uint32_t m = (eq << 8) - eq;                         // 0xFF per equal byte
            const uint32_t m0 = __builtin_amdgcn_perm(m, m, 0x01010000u), m1 = __builtin_amdgcn_perm(m, m, 0x03030202u);
            const uint32_t h0 = hw_[2 * hw] & m0, h1 = hw_[2 * hw + 1] & m1, l0 = lw_[2 * hw] & m0, l1 = lw_[2 * hw + 1] & m1;
            g[4 * hw + 0] += __uint_as_float(h0 << 16) + __uint_as_float(l0 << 16);                   // hi + lo is exact in fp32
            g[4 * hw + 1] += __uint_as_float(h0 & 0xFFFF0000u) + __uint_as_float(l0 & 0xFFFF0000u);
            g[4 * hw + 2] += __uint_as_float(h1 << 16) + __uint_as_float(l1 << 16);
            g[4 * hw + 3] += __uint_as_float(h1 & 0xFFFF0000u) + __uint_as_float(l1 & 0xFFFF0000u);
          }
        }
      }
    }
    uint32_t hv[4], lv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      hv[k] = pack_bf16x2(g[2 * k], g[2 * k + 1]);
      lv[k] = pack_bf16x2(g[2 * k] - __uint_as_float(hv[k] << 16), g[2 * k + 1] - __uint_as_float(hv[k] & 0xFFFF0000u));
    }
    sDz1[c * NPOS_PAD + hy * HT + hx] = make_uint4(hv[0], hv[1], hv[2], hv[3]);
    sDz1[(4 + c) * NPOS_PAD + hy * HT + hx] = make_uint4(lv[0], lv[1], lv[2], lv[3]);
  }
}


__global__ __launch_bounds__(256, 2) void k_stem_bwd_pair(const uint4* __restrict__ dpool_h,    // [n][oh2][ow2][64] bf16, hi plane
                                                          const uint4* __restrict__ dpool_l,    // lo plane
                                                          const uint4* __restrict__ arg,        // [n][oh2][ow2][64] u8 codes
                                                          const uint16_t* __restrict__ wt_h,    // [16][1024] bf16 (stem_fused.hip's table), hi
                                                          const uint16_t* __restrict__ wt_l,    // lo
                                                          float* __restrict__ grad,             // [n][3][h][w]
                                                          int h, int w, RartIstd3 istd) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[DZ_BYTES + RW_BYTES];
  uint4* sDz1 = reinterpret_cast<uint4*>(lds);                                     // [2][4][NPOS_PAD]
  uint4* sDp = reinterpret_cast<uint4*>(lds + DZ_BYTES);                           // [2][NPOOL_PAD][4] (window-major)
  uint2* sArg = reinterpret_cast<uint2*>(lds + DZ_BYTES + DP_BYTES);               // [NPOOL_PAD][4]
  uint4* sW = reinterpret_cast<uint4*>(lds + DZ_BYTES);                            // [2][16][64] (aliases the raw tile, dead by then)
  float* sOut = reinterpret_cast<float*>(lds + DZ_BYTES);                          // [3][OPL] rows of OLD (aliases the weights, dead by then)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int oh = h >> 1, ow = w >> 1;            // stem-output grid
  const int oh2 = oh >> 1, ow2 = ow >> 1;        // pooled grid
  const int a0 = blockIdx.y * T, b0 = blockIdx.x * T, img = blockIdx.z;
  const int qy0 = (a0 >> 1) - 1, qx0 = (b0 >> 1) - 1;      // first pooled row / column that reaches the halo tile
  const int fr = lane & 15, fg = lane >> 4;
  f32x4 acc[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // a wave's B fragment of a tap is 1 KiB of the table (row fr, 8 channels at fg * 8 of the tap's channel half): the workgroup fetches
  // the 2 x 16 fragments of a half ONCE into LDS in fragment order (lane-contiguous: conflict free) instead of once per wave
  const uint4* wsrc_h = reinterpret_cast<const uint4*>(wt_h + (size_t)fr * 1024 + fg * 8) + wave * 8;   // taps wave, wave + 4, ... (+ half * 4)
  const uint4* wsrc_l = reinterpret_cast<const uint4*>(wt_l + (size_t)fr * 1024 + fg * 8) + wave * 8;

  // the raw pooled tile of a channel half (121 windows x (8 gradient chunks + 2 code chunks) of 16 bytes): every load of a half is
  // requested before the first is used, and the second half's before the matrix phase of the first -- a load per loop pass, waited for
  // one after the other, left five exposed latencies per half
  constexpr int SU = (NPOOL * 10 + 255) / 256;
  uint4 sv[SU];
  auto load_raw = [&](int half) {
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int i = u * 256 + tid;
      const int pos = i / 10, v = i - pos * 10;
      const int ry = pos / PT, rx = pos - ry * PT;
      const int qy = qy0 + ry, qx = qx0 + rx;
      const bool ok = i < NPOOL * 10 && (unsigned)qy < (unsigned)oh2 && (unsigned)qx < (unsigned)ow2;
      const size_t base = ((size_t)img * oh2 + qy) * ow2 + qx;
      sv[u] = v < 8 ? make_uint4(0, 0, 0, 0) : make_uint4(0x0F0F0F0Fu, 0x0F0F0F0Fu, 0x0F0F0F0Fu, 0x0F0F0F0Fu);
      if (ok) sv[u] = v < 8 ? ((v >> 2) ? dpool_l : dpool_h)[base * 8 + half * 4 + (v & 3)] : arg[base * 4 + half * 2 + (v - 8)];
    }
  };
  SP_ST(unsigned long long st[4] = {0, 0, 0, 0};)
  SP_T(tb)
  load_raw(0);
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    SP_T(t0)
    // ---- stage the pooled gradient pair and the argmax codes of this channel half (zeros / code 15 outside the grid)
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int i = u * 256 + tid;
      if (i >= NPOOL * 10) continue;
      const int pos = i / 10, v = i - pos * 10;
      const int ry = pos / PT, lp = ry * PTS + (pos - ry * PT);
      if (v < 8) {
        sDp[((v >> 2) * NPOOL_PAD + lp) * 4 + (v & 3)] = sv[u];
      } else {
        sArg[lp * 4 + 2 * (v - 8)] = make_uint2(sv[u].x, sv[u].y);
        sArg[lp * 4 + 2 * (v - 8) + 1] = make_uint2(sv[u].z, sv[u].w);
      }
    }
    __syncthreads();
    SP_T(t1)
    // ---- max-pool backward into the halo tile, one pass per pixel-parity class
    pool_bwd_class_pair<0, 0>(sDz1, sDp, sArg, tid, a0, b0, qy0, qx0, oh, ow);
    pool_bwd_class_pair<0, 1>(sDz1, sDp, sArg, tid, a0, b0, qy0, qx0, oh, ow);
    pool_bwd_class_pair<1, 0>(sDz1, sDp, sArg, tid, a0, b0, qy0, qx0, oh, ow);
    pool_bwd_class_pair<1, 1>(sDz1, sDp, sArg, tid, a0, b0, qy0, qx0, oh, ow);
    __syncthreads();
    SP_T(t2)
    // ---- the weight fragments of this half into the region the raw tile just left: wave w brings taps w, w + 4, w + 8, w + 12
    {
      uint4 th[4], tl[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        th[k] = wsrc_h[k * 32 + half * 4];
        tl[k] = wsrc_l[k * 32 + half * 4];
      }
      if (half == 0) load_raw(1);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        sW[(wave + 4 * k) * 64 + lane] = th[k];
        sW[(16 + wave + 4 * k) * 64 + lane] = tl[k];
      }
    }
    __syncthreads();
    // ---- implicit GEMM over the 16 taps of this channel half: wave w owns tile rows 4w..4w+3 (one 16-position M tile each)
#pragma unroll
    for (int dpi = 0; dpi < 4; ++dpi) {
#pragma unroll
      for (int dqi = 0; dqi < 4; ++dqi) {
        const bf16x8 wh = __builtin_bit_cast(bf16x8, sW[(dpi * 4 + dqi) * 64 + lane]);
        const bf16x8 wl = __builtin_bit_cast(bf16x8, sW[(16 + dpi * 4 + dqi) * 64 + lane]);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int pos = (wave * 4 + m + dpi) * HT + fr + dqi;
          const bf16x8 ah = __builtin_bit_cast(bf16x8, sDz1[fg * NPOS_PAD + pos]);
          const bf16x8 al = __builtin_bit_cast(bf16x8, sDz1[(4 + fg) * NPOS_PAD + pos]);
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wh, acc[m], 0, 0, 0);
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wl, acc[m], 0, 0, 0);
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wh, acc[m], 0, 0, 0);
        }
      }
    }
    __syncthreads();                     // the weights are dead: the next half's raw tile, or the output tile, takes their place
    SP_T(t3)
    SP_ST(st[0] += t1 - t0; st[1] += t2 - t1; st[2] += t3 - t2;)
  }

  // ---- epilogue: D[row = fg*4 + j (position column)][col = fr = (py*2+px)*3 + c] -> sOut[c][2a+py][2b+px]
  //      (the weights are dead: every wave passed the barrier after its last read of them)
  SP_T(t4)
  if (fr < 12) {
    const int pq = fr / 3, c = fr - pq * 3;
    const int py = pq >> 1, px = pq & 1;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        sOut[c * OPL + (2 * (wave * 4 + m) + py) * OLD + 2 * (fg * 4 + j) + px] = acc[m][j];
  }
  __syncthreads();
  const size_t plane = (size_t)h * w;
  for (int i = tid; i < 3 * OT * (OT / 4); i += 256) {
    const int x4 = i & 7, row = i >> 3;
    const int c = row / OT, y = row - c * OT;
    const int gy = 2 * a0 + y, gx = 2 * b0 + x4 * 4;
    if (gy < h && gx < w) {
      const float s = istd.v[c];
      const float* r = sOut + c * OPL + y * OLD + x4 * 4;
      *reinterpret_cast<float4*>(grad + ((size_t)img * 3 + c) * plane + (size_t)gy * w + gx) =
          make_float4(r[0] * s, r[1] * s, r[2] * s, r[3] * s);
    }
  }
  SP_T(t6)
  SP_ST(if (lane == 0) {
    for (int k = 0; k < 3; ++k) atomicAdd(&g_sp_stamps[0][k], st[k]);
    atomicAdd(&g_sp_stamps[0][3], t6 - t4);
    atomicAdd(&g_sp_stamps[0][4], t6 - tb);
    atomicAdd(&g_sp_stamps[0][5], 1ull);
  })
}
}  // namespace

extern "C" int rart_engine_stem_bwd_fused_pair(const void* dpool_hi, const void* dpool_lo, const void* argmax, const void* wtab_hi,
                                               const void* wtab_lo, float* grad, int n, int h, int w, const float* std_host,
                                               rart_stream_t stream) {
  RART_CHECK_ARG(dpool_hi && dpool_lo && argmax && wtab_hi && wtab_lo && grad && n > 0 && n <= 65535,
                 "rart_engine_stem_bwd_fused_pair: bad arguments");
  RART_CHECK_ARG(h % 4 == 0 && w % 4 == 0 && h >= 4 && w >= 4, "rart_engine_stem_bwd_fused_pair: h and w must be multiples of 4");
  const RartIstd3 is = rart_istd3(std_host);
  const int oh = h / 2, ow = w / 2;
  hipLaunchKernelGGL(k_stem_bwd_pair, dim3((ow + T - 1) / T, (oh + T - 1) / T, n), dim3(256), 0, (hipStream_t)stream,
                     (const uint4*)dpool_hi, (const uint4*)dpool_lo, (const uint4*)argmax, (const uint16_t*)wtab_hi,
                     (const uint16_t*)wtab_lo, grad, h, w, is);
  RART_CHECK_LAUNCH("rart_engine_stem_bwd_fused_pair");
  return RART_OK;
}

// =====================================================================================================================
// Fused stem FORWARD on pairs: input normalisation (hi + lo bf16 split) + 7x7/2 convolution (x_lo.w_hi + x_hi.w_lo + x_hi.w_hi per K
// step, fp32 accumulation) + folded BatchNorm bias + ReLU + hi + lo split + 3x3/2 max pool of the pair VALUES in ONE persistent kernel.
// Replaces rart_engine_prep_input -> rart_gemm_pair_bf16 (row taps, K = 224) -> rart_engine_maxpool_pair, which wrote and re-read the
// padded hi / lo image and the 112 x 112 x 64 stem-output pair (2 x 411 MB per 256 images): 0.77 ms of a 10.1 ms forward.
//
// Same structure as k_stem_fwd_fused (csrc/stem_fused.hip): a workgroup loops over 8 x 8 tiles of POOLED positions; the 39 x 39 input
// patch behind the 17 x 17 stem outputs the tile's windows touch is staged in LDS as two planes of 39 rows of [40 px][4 ch] bf16 (rows in
// pairs of 784 bytes, see SP_PW); the convolution
// is the row-tap implicit GEMM (a tap = one filter row of 8 px x 4 ch) read straight from the patch, operands swapped so a lane owns 4
// consecutive channels of one position.  What the pair changes: both weight planes are LDS resident (2 x 29.7 KB), and the stem-output
// tile is kept as fp32 -- the value hi + lo of the pair the unfused chain would have written, so the pool's comparisons, argmax codes and
// outputs are bit-identical to it -- 78.6 KB: one workgroup of 512 threads per CU (138 KB of LDS).
//
// NEXT instances (rart_engine_stem_fwd_next_pair): layer1 block 0's conv1 (1x1, 64 -> 64) + bias + ReLU on the pooled tile before it leaves
// the CU -- that launch (802816 x 64 -> 64 at B = 256) re-read the 205 MB pooled pair this kernel has just written.  Both planes of its
// 64 x 64 table stay LDS resident beside the stem's (2 x 9 KB, rows of SP_NROW bytes); after the pool the tile's 64 pooled positions go to
// LDS as the pair this kernel stores (hi, lo of the same rounding: the operand the separate launch reads), waves 0-3 run one 32 x 32 block
// each -- accumulators start at the bias, per 16-deep K slice a_lo.w_hi, a_hi.w_lo, a_hi.w_hi: k_gemm_pair's products in k_gemm_pair's
// order, so the output pair and its sign bits are the separate launch's bit for bit -- and the fp32 block goes through LDS to the pool's
// thread mapping (one position x 8 channels per thread) for ReLU, the hi / lo split and 16-byte stores.  156 432 B of LDS.
// =====================================================================================================================
namespace {
constexpr int SP_PT = 8;                        // pooled tile side
constexpr int SP_R = 2 * SP_PT + 1;             // stem-output region side (17)
constexpr int SP_NPOS = SP_R * SP_R;            // 289
constexpr int SP_PH = 2 * (SP_R - 1) + 7;       // patch rows (39)
constexpr int SP_SW = 40;                       // pixels staged per patch row (39 + the zero column the 8th pixel of the last tap reads)
constexpr int SP_PW = 49;                       // stride of a PAIR of patch rows in 16-byte slots: = 1 mod 16, so going from the 17th position
                                                // of a row to the 1st of the next (two patch rows down) continues the bank sequence and an A
                                                // fragment read is conflict free.  A single-row stride of 49 pixels would put the odd row
                                                // taps 8 bytes off the 16-byte alignment of the fragment reads (ds_read_b128), so the odd row of a pair
                                                // sits SP_ODD bytes into it instead
constexpr int SP_ODD = 400;                     // byte offset of the odd patch row in its pair (>= SP_SW * 8, a multiple of 16)
constexpr int SP_PLANE = (SP_PH + 1) / 2 * SP_PW * 16;     // bytes per hi / lo plane (15 680)
// (SP_PW, SP_ODD, SP_R and the fragment addresses are mirrored in tests/test_stem_pair_bank_model.py)
__device__ __forceinline__ constexpr int sp_row_off(int row) { return (row >> 1) * (SP_PW * 16) + (row & 1) * SP_ODD; }
static_assert(SP_ODD % 16 == 0 && SP_ODD >= SP_SW * 8 && SP_PW * 16 - SP_ODD >= SP_SW * 8, "both rows of a pair fit its stride");
constexpr int SP_WROW = 464;                    // weight row stride in LDS (224 k x 2 B + 16 pad: conflict-free b128 reads)
constexpr int SP_YROW = 272;                    // stem-output tile row stride: 64 fp32 + 16 B pad
constexpr int SP_W_BYTES = 64 * SP_WROW;        // 29 696 per plane
constexpr int SP_T_BYTES = SP_NPOS * SP_YROW;   // 78 608 (>= 2 * SP_PLANE: the tile aliases the patch)
constexpr int SP_NT = 3;                        // 32-position M tiles of wave rows 0 and 1; wave rows 2 and 3 take 2: 10 tiles cover the 289
                                                // positions, and every SIMD holds one wave of each kind (waves w and w + 4)
constexpr int SP_U = (SP_PH * SP_SW + 511) / 512;   // patch pixels a thread stages per tile (4)
static_assert(SP_T_BYTES >= 2 * SP_PLANE, "the stem-output tile must cover the patch it aliases");
// NEXT: the 64 x 64 table planes and the pooled tile's planes as rows of 64 bf16 + 16 B (conflict-free b128 fragment reads); the pooled
// planes and the fp32 result block [64 positions][SP_YROW] alias the stem-output tile once the pool has read it
constexpr int SP_NROW = 144;
constexpr int SP_N_BYTES = 64 * SP_NROW;        // 9 216 per plane
static_assert(2 * SP_N_BYTES + 64 * SP_YROW <= SP_T_BYTES, "pooled planes + result block fit the tile they alias");
static_assert(2 * SP_W_BYTES + SP_T_BYTES + 2 * SP_N_BYTES <= 160 * 1024, "one workgroup per CU");

// the normalisation must round exactly like k_prep_input (engine_aux.hip): multiply, subtract, multiply -- no contraction
#pragma clang fp contract(off)

struct StemNextP {          // NEXT: the 1x1 that follows the pool -- table planes [64][ldw] bf16, bias, output pair [pos][64], its sign bits
  const uint16_t *w_h, *w_l;
  const float* bias;
  uint4 *y_h, *y_l;
  uint8_t* sign;
  int ldw;
};

template <bool SRC_U8, bool NEXT = false>
__global__ __launch_bounds__(512, 1) void k_stem_fwd_pair(const void* __restrict__ src, const uint16_t* __restrict__ w_h,
                                                          const uint16_t* __restrict__ w_l, const float* __restrict__ bias,
                                                          uint4* __restrict__ p1_h, uint4* __restrict__ p1_l, uint2* __restrict__ arg,
                                                          uint8_t* __restrict__ sign, int n, int h, int w, RartNorm3 nm, StemNextP nx) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * SP_W_BYTES + SP_T_BYTES + (NEXT ? 2 * SP_N_BYTES : 0)];
  uint8_t* sW = lds;                            // [hi | lo][64][SP_WROW]
  uint8_t* sP = lds + 2 * SP_W_BYTES;           // patch (hi plane, lo plane) / stem-output tile
  uint8_t* sN = lds + 2 * SP_W_BYTES + SP_T_BYTES;      // NEXT: [hi | lo][64][SP_NROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int kq = lane >> 5;
  const int oh = h >> 1, ow = w >> 1, oh2 = oh >> 1, ow2 = ow >> 1;
  const int tiles_x = (ow2 + SP_PT - 1) / SP_PT, tiles_y = (oh2 + SP_PT - 1) / SP_PT;
  const int n_tiles = n * tiles_y * tiles_x;

  // weights: [64][224] per plane, once per workgroup
  for (int i = tid; i < 2 * 64 * 28; i += 512) {
    const int pl = i / (64 * 28), j = i - pl * (64 * 28), row = j / 28, ch = j - row * 28;
    *reinterpret_cast<uint4*>(sW + pl * SP_W_BYTES + row * SP_WROW + ch * 16) =
        *reinterpret_cast<const uint4*>((pl ? w_l : w_h) + (size_t)row * 224 + ch * 8);
  }
  float bzn[16];
  if (NEXT) {
    for (int i = tid; i < 2 * 64 * 8; i += 512) {
      const int pl = i >> 9, j = i & 511, row = j >> 3, ch = j & 7;
      *reinterpret_cast<uint4*>(sN + pl * SP_N_BYTES + row * SP_NROW + ch * 16) =
          *reinterpret_cast<const uint4*>((pl ? nx.w_l : nx.w_h) + (size_t)row * nx.ldw + ch * 8);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) bzn[r] = nx.bias ? nx.bias[(wave & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kq] : 0.f;
  }
  const int mt0 = wm < 2 ? wm * SP_NT : 2 * SP_NT + (wm - 2) * (SP_NT - 1);     // first M tile of this wave row: 0, 3, 6, 8
  const int n_mt = wm < 2 ? SP_NT : SP_NT - 1;
  uint32_t a_off[SP_NT];
#pragma unroll
  for (int i = 0; i < SP_NT; ++i) {
    int p = (mt0 + i) * 32 + (lane & 31);
    p = p < SP_NPOS ? p : SP_NPOS - 1;          // rows past the region recompute the last position; never stored
    const int py = p / SP_R, px = p - py * SP_R;
    a_off[i] = (uint32_t)(py * (SP_PW * 16) + 2 * px * 8 + kq * 16);
  }
  const uint32_t w_off = (uint32_t)((wn * 32 + (lane & 31)) * SP_WROW + kq * 16);
  float bz[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) bz[r] = bias ? bias[wn * 32 + (r & 3) + 8 * (r >> 2) + 4 * kq] : 0.f;

  // the source values of a tile's patch (4 pixels x 3 values per thread).  The fp32 instance requests them one tile ahead: the loads of
  // tile t + gridDim.x are issued before the matrix phase of tile t and held in registers until the loop top normalises, splits and
  // writes them.  The uint8 instance loads at the loop top: with its byte loads beside the MFMAs it measured slower ("Stem
  // pair kernels", has the figures)
  constexpr bool PREFETCH = !SRC_U8 || RART_STEM_U8_PREFETCH;
  float v01[SP_U][3];
  bool ok[SP_U];
  auto load_patch = [&](int t) {
    const int img = t / (tiles_y * tiles_x);
    const int tr = t - img * (tiles_y * tiles_x);
    const int in_y0 = 4 * ((tr / tiles_x) * SP_PT) - 5, in_x0 = 4 * ((tr % tiles_x) * SP_PT) - 5;      // input pixel of patch (0, 0)
#pragma unroll
    for (int u = 0; u < SP_U; ++u) {
      const int i = u * 512 + tid;
      const int pr = i / SP_SW, pc = i - pr * SP_SW;
      const int y = in_y0 + pr, x = in_x0 + pc;
      ok[u] = t < n_tiles && i < SP_PH * SP_SW && (unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w && pc < SP_PH;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v01[u][c] = 0.f;
        if (ok[u]) {
          if (SRC_U8) v01[u][c] = (float)((const uint8_t*)src)[(((size_t)img * h + y) * w + x) * 3 + c];
          else v01[u][c] = ((const float*)src)[(((size_t)img * 3 + c) * h + y) * w + x];
        }
      }
    }
  };
  if (PREFETCH) load_patch(blockIdx.x);

  SP_ST(unsigned long long fs[6] = {0, 0, 0, 0, 0, 0};)
  SP_T(tf0)
  for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int img = t / (tiles_y * tiles_x);
    const int tr = t - img * (tiles_y * tiles_x);
    const int q0y = (tr / tiles_x) * SP_PT, q0x = (tr % tiles_x) * SP_PT;
    if (!PREFETCH) load_patch(t);
    SP_T(t0)
    __syncthreads();                                               // previous tile's pool is done with the LDS tile
    // ---- stage the patch: (x - mean) / std as hi + lo bf16, zeros outside the image and in the 4th channel
#pragma unroll
    for (int u = 0; u < SP_U; ++u) {
      const int i = u * 512 + tid;
      if (i >= SP_PH * SP_SW) continue;
      const int pr = i / SP_SW, po = sp_row_off(pr) + (i - pr * SP_SW) * 8;
      uint32_t hv[3] = {0, 0, 0}, lv[3] = {0, 0, 0};
      if (ok[u]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float x01 = SRC_U8 ? v01[u][c] * (1.0f / 255.0f) : v01[u][c];
          const float v = (x01 - nm.mean[c]) * nm.istd[c];
          hv[c] = pack_bf16x2(v, 0.f) & 0xFFFFu;
          lv[c] = pack_bf16x2(v - __uint_as_float(hv[c] << 16), 0.f) & 0xFFFFu;
        }
      }
      *reinterpret_cast<uint2*>(sP + po) = make_uint2(hv[0] | (hv[1] << 16), hv[2]);
      *reinterpret_cast<uint2*>(sP + SP_PLANE + po) = make_uint2(lv[0] | (lv[1] << 16), lv[2]);
    }
    __syncthreads();
    SP_T(t1)
    if (PREFETCH) load_patch(t + gridDim.x);                       // the next tile's source (nothing past the last tile)
    // ---- implicit GEMM: 7 row taps x 2 k-steps x 3 products, D^T accumulators (register -> channel, lane -> position)
    f32x16 acc[SP_NT];
#pragma unroll
    for (int i = 0; i < SP_NT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = bz[r];
    auto row_taps = [&](auto nt) {                                 // (the tile count is a compile-time constant of each instance)
#pragma unroll
      for (int r = 0; r < 7; ++r)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8 wh = *reinterpret_cast<const bf16x8*>(sW + w_off + r * 64 + ks * 32);
          const bf16x8 wl = *reinterpret_cast<const bf16x8*>(sW + SP_W_BYTES + w_off + r * 64 + ks * 32);
#pragma unroll
          for (int i = 0; i < decltype(nt)::value; ++i) {
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(sP + a_off[i] + sp_row_off(r) + ks * 32);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(sP + a_off[i] + SP_PLANE + sp_row_off(r) + ks * 32);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, al, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, ah, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, ah, acc[i], 0, 0, 0);
          }
        }
    };
    if (wm < 2) row_taps(std::integral_constant<int, SP_NT>());
    else row_taps(std::integral_constant<int, SP_NT - 1>());
    SP_T(t2)
    __syncthreads();                                               // every wave is done reading the patch
    SP_T(t3)
    // ---- ReLU, the value of the hi + lo pair (what the unfused chain stores), into the LDS tile [position][64 ch] fp32
#pragma unroll
    for (int i = 0; i < SP_NT; ++i) {
      const int p = (mt0 + i) * 32 + (lane & 31);
      if (i < n_mt && p < SP_NPOS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = fmaxf(acc[i][4 * q + k], 0.f);
          const uint32_t h0 = pack_bf16x2(v[0], v[1]), h1 = pack_bf16x2(v[2], v[3]);
          const uint32_t l0 = pack_bf16x2(v[0] - __uint_as_float(h0 << 16), v[1] - __uint_as_float(h0 & 0xFFFF0000u));
          const uint32_t l1 = pack_bf16x2(v[2] - __uint_as_float(h1 << 16), v[3] - __uint_as_float(h1 & 0xFFFF0000u));
          *reinterpret_cast<float4*>(sP + p * SP_YROW + (wn * 32 + 8 * q + 4 * kq) * 4) =
              make_float4(__uint_as_float(h0 << 16) + __uint_as_float(l0 << 16), __uint_as_float(h0 & 0xFFFF0000u) + __uint_as_float(l0 & 0xFFFF0000u),
                          __uint_as_float(h1 << 16) + __uint_as_float(l1 << 16), __uint_as_float(h1 & 0xFFFF0000u) + __uint_as_float(l1 & 0xFFFF0000u));
        }
      }
    }
    __syncthreads();
    SP_T(t4)
    // ---- 3x3/2 max pool (pad 1) of the pair values: first maximum in scan order, code 15 when the maximum is <= 0
    {
      const int c = tid & 7, q = tid >> 3;          // 64 pooled positions x 8 channel groups = 512 threads
      const int qy = q / SP_PT, qx = q - qy * SP_PT;
      const int gy = q0y + qy, gx = q0x + qx;
      uint4 nh = make_uint4(0, 0, 0, 0), nl = nh;   // NEXT: this thread's 8 channels of the pooled pair (zeros outside the grid)
      if (gy < oh2 && gx < ow2) {
        float m[8];
        uint32_t code[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { m[j] = -INFINITY; code[j] = 0; }
        for (int ky = 0; ky < 3; ++ky) {
          const int y1 = 2 * gy - 1 + ky;
          if ((unsigned)y1 >= (unsigned)oh) continue;
          for (int kx = 0; kx < 3; ++kx) {
            const int x1 = 2 * gx - 1 + kx;
            if ((unsigned)x1 >= (unsigned)ow) continue;
            const float* tp = reinterpret_cast<const float*>(sP + ((2 * qy + ky) * SP_R + 2 * qx + kx) * SP_YROW) + c * 8;
            const float4 v0 = *reinterpret_cast<const float4*>(tp), v1 = *reinterpret_cast<const float4*>(tp + 4);
            const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (f[j] > m[j]) { m[j] = f[j]; code[j] = (uint32_t)(ky * 3 + kx); }
          }
        }
        const size_t o = (((size_t)img * oh2 + gy) * ow2 + gx) * 8 + c;
        uint32_t hv[4], lv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          hv[k] = pack_bf16x2(m[2 * k], m[2 * k + 1]);
          lv[k] = pack_bf16x2(m[2 * k] - __uint_as_float(hv[k] << 16), m[2 * k + 1] - __uint_as_float(hv[k] & 0xFFFF0000u));
        }
        p1_h[o] = make_uint4(hv[0], hv[1], hv[2], hv[3]);
        p1_l[o] = make_uint4(lv[0], lv[1], lv[2], lv[3]);
        if (NEXT) { nh = make_uint4(hv[0], hv[1], hv[2], hv[3]); nl = make_uint4(lv[0], lv[1], lv[2], lv[3]); }
        uint32_t sb = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (m[j] > 0.f) sb |= 1u << j; else code[j] = 15u;
        }
        if (sign) sign[o] = (uint8_t)sb;
        if (arg) arg[o] = make_uint2(code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24),
                                     code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24));
      }
      if (NEXT) {
        // ---- the 1x1 that follows: y = relu(W . p1 + b) on the tile's 64 pooled positions
        __syncthreads();                                             // every thread is done reading the stem-output tile
        *reinterpret_cast<uint4*>(sP + q * SP_NROW + c * 16) = nh;
        *reinterpret_cast<uint4*>(sP + SP_N_BYTES + q * SP_NROW + c * 16) = nl;
        __syncthreads();
        float* const sY = reinterpret_cast<float*>(sP + 2 * SP_N_BYTES);
        if (wave < 4) {                                              // 2 x 2 blocks of 32 positions x 32 channels
          const int pm = wave >> 1, pn = wave & 1;
          const uint8_t* ap = sP + (pm * 32 + (lane & 31)) * SP_NROW + kq * 16;
          const uint8_t* wp = sN + (pn * 32 + (lane & 31)) * SP_NROW + kq * 16;
          f32x16 an;
#pragma unroll
          for (int r = 0; r < 16; ++r) an[r] = bzn[r];
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 wh = *reinterpret_cast<const bf16x8*>(wp + ks * 32), wl = *reinterpret_cast<const bf16x8*>(wp + SP_N_BYTES + ks * 32);
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(ap + ks * 32), al = *reinterpret_cast<const bf16x8*>(ap + SP_N_BYTES + ks * 32);
            an = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, al, an, 0, 0, 0);
            an = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, ah, an, 0, 0, 0);
            an = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, ah, an, 0, 0, 0);
          }
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4)
            *reinterpret_cast<float4*>(reinterpret_cast<uint8_t*>(sY) + (pm * 32 + (lane & 31)) * SP_YROW + (pn * 32 + 8 * g4 + 4 * kq) * 4) =
                make_float4(an[4 * g4], an[4 * g4 + 1], an[4 * g4 + 2], an[4 * g4 + 3]);
        }
        __syncthreads();
        if (gy < oh2 && gx < ow2) {
          const float* yp = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(sY) + q * SP_YROW) + c * 8;
          const float4 v0 = *reinterpret_cast<const float4*>(yp), v1 = *reinterpret_cast<const float4*>(yp + 4);
          const float f[8] = {fmaxf(v0.x, 0.f), fmaxf(v0.y, 0.f), fmaxf(v0.z, 0.f), fmaxf(v0.w, 0.f),
                              fmaxf(v1.x, 0.f), fmaxf(v1.y, 0.f), fmaxf(v1.z, 0.f), fmaxf(v1.w, 0.f)};
          uint32_t hv[4], lv[4], sb = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            hv[k] = pack_bf16x2(f[2 * k], f[2 * k + 1]);
            lv[k] = pack_bf16x2(f[2 * k] - __uint_as_float(hv[k] << 16), f[2 * k + 1] - __uint_as_float(hv[k] & 0xFFFF0000u));
            sb |= ((short)(hv[k] & 0xFFFFu) > 0 ? 1u : 0u) << (2 * k);          // (hi plane > 0), as the pair GEMM's epilogue writes it
            sb |= ((short)(hv[k] >> 16) > 0 ? 1u : 0u) << (2 * k + 1);
          }
          const size_t o = (((size_t)img * oh2 + gy) * ow2 + gx) * 8 + c;
          nx.y_h[o] = make_uint4(hv[0], hv[1], hv[2], hv[3]);
          nx.y_l[o] = make_uint4(lv[0], lv[1], lv[2], lv[3]);
          if (nx.sign) nx.sign[o] = (uint8_t)sb;
        }
      }
    }
    SP_T(t5)
    SP_ST(fs[0] += t1 - t0; fs[1] += t2 - t1; fs[2] += t3 - t2; fs[3] += t4 - t3; fs[4] += t5 - t4; fs[5] += 1;)
  }
  SP_T(tf1)
  SP_ST(if (lane == 0) {
    for (int k = 0; k < 6; ++k) atomicAdd(&g_sp_stamps[1][k], fs[k]);
    atomicAdd(&g_sp_stamps[1][6], tf1 - tf0);
    atomicAdd(&g_sp_stamps[1][7], 1ull);
  })
}
#pragma clang fp contract(fast)
}  // namespace

static int stem_fwd_pair_launch(const void* src, int src_is_u8, const void* wgt_hi, const void* wgt_lo, const float* bias, void* p1_hi,
                                void* p1_lo, void* argmax_out, void* sign_out, int n, int h, int w, const float* mean_host,
                                const float* std_host, rart_stream_t stream, const StemNextP* next) {
  RART_CHECK_ARG(src && wgt_hi && wgt_lo && p1_hi && p1_lo && n > 0 && h % 4 == 0 && w % 4 == 0 && h >= 4 && w >= 4,
                 "rart_engine_stem_fwd_fused_pair: bad arguments (h, w multiples of 4)");
  const RartNorm3 nm = rart_norm3(mean_host, std_host);
  const long long tiles = (long long)n * ((h / 4 + SP_PT - 1) / SP_PT) * ((w / 4 + SP_PT - 1) / SP_PT);
  const int grid = (int)(tiles < 256 ? tiles : 256);              // persistent: one workgroup per CU
#define RART_STEM_LAUNCH(U8_, NEXT_)                                                                                         \
  hipLaunchKernelGGL((k_stem_fwd_pair<U8_, NEXT_>), dim3(grid), dim3(512), 0, (hipStream_t)stream, src, (const uint16_t*)wgt_hi, \
                     (const uint16_t*)wgt_lo, bias, (uint4*)p1_hi, (uint4*)p1_lo, (uint2*)argmax_out, (uint8_t*)sign_out, n, h, w, nm, nx)
  const StemNextP nx = next ? *next : StemNextP{};
  if (next) {
    if (src_is_u8) RART_STEM_LAUNCH(true, true);
    else RART_STEM_LAUNCH(false, true);
  } else {
    if (src_is_u8) RART_STEM_LAUNCH(true, false);
    else RART_STEM_LAUNCH(false, false);
  }
#undef RART_STEM_LAUNCH
  RART_CHECK_LAUNCH("rart_engine_stem_fwd_fused_pair");
  return RART_OK;
}

extern "C" int rart_engine_stem_fwd_fused_pair(const void* src, int src_is_u8, const void* wgt_hi, const void* wgt_lo, const float* bias,
                                               void* p1_hi, void* p1_lo, void* argmax_out, void* sign_out, int n, int h, int w,
                                               const float* mean_host, const float* std_host, rart_stream_t stream) {
  return stem_fwd_pair_launch(src, src_is_u8, wgt_hi, wgt_lo, bias, p1_hi, p1_lo, argmax_out, sign_out, n, h, w, mean_host, std_host, stream,
                              nullptr);
}

// ... and the 1x1 convolution (64 -> 64) + bias + ReLU that reads the pooled pair, on the tile before it leaves the CU (NEXT instances).
extern "C" int rart_engine_stem_fwd_next_pair(const void* src, int src_is_u8, const void* wgt_hi, const void* wgt_lo, const float* bias,
                                              void* p1_hi, void* p1_lo, void* argmax_out, void* sign_out, const void* wnext_hi,
                                              const void* wnext_lo, int ldw_next, const float* bias_next, void* next_hi, void* next_lo,
                                              void* next_sign_out, int n, int h, int w, const float* mean_host, const float* std_host,
                                              rart_stream_t stream) {
  RART_CHECK_ARG(wnext_hi && wnext_lo && next_hi && next_lo && ldw_next >= 64 && ldw_next % 8 == 0,
                 "rart_engine_stem_fwd_next_pair: the next 1x1 needs both table planes ([64][ldw_next], ldw_next >= 64, a multiple of 8) and "
                 "both output planes");
  const StemNextP nx = {(const uint16_t*)wnext_hi, (const uint16_t*)wnext_lo, bias_next, (uint4*)next_hi, (uint4*)next_lo,
                        (uint8_t*)next_sign_out, ldw_next};
  return stem_fwd_pair_launch(src, src_is_u8, wgt_hi, wgt_lo, bias, p1_hi, p1_lo, argmax_out, sign_out, n, h, w, mean_host, std_host, stream,
                              &nx);
}

#ifdef RART_STEM_STAMPS
extern "C" int rart_debug_stem_stamps(unsigned long long* out16, int reset) {
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_sp_stamps), sizeof(unsigned long long) * 16) != hipSuccess) return 1;
  if (reset) {
    unsigned long long z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_sp_stamps), z, sizeof(z)) != hipSuccess) return 1;
  }
  return 0;
}
#endif
