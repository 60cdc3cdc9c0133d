// Split-bf16 ("fp32x" / "bf16x3") GEMM for gfx950 (CDNA4): the dense contraction of the REFERENCE-PRECISION engines.
//
//   C[m][n] = sum_k A[m][k] * W[n][k]      A = A_hi + A_lo, W = W_hi + W_lo (each a plane of bf16 values)
//   A.W ~= A_lo.W_hi + A_hi.W_lo + A_hi.W_hi   (the dropped lo.lo term is 2^-16 of a product), fp32 accumulation
//
// The reference computes fp32 everywhere (RobustART/noise/utils/adv/attack.py:20-23 wraps an fp32 f_model;
// Attacks/autoattack/autopgd_base.py:271-289 takes fp32 logits and gradients; exprs/exp/imagenet_c_loop_mini/config_vit_base.yaml:1-9
// has no precision key) and the north star asks for logits within 1e-4 of it.  gfx950's fp32 MFMA peaks at 157 TFLOP/s, its bf16
// MFMA at 2 500: three bf16 products per algorithmic product are 5 x faster than fp32 operands.
//
// Round 3 ran this scheme on the implicit-GEMM kernel by listing the three products as 3 x the taps: every product stages its own
// A and W tiles (x_hi is fetched and written to LDS twice).  This kernel stages the FOUR operand planes of a K step once and issues
// the three MFMAs per fragment pair from them: 2/3 of the global -> LDS traffic and of the ds_read traffic per MFMA.
//
// Design for MI355X: 256 x 256 tile, 8 wave64s each owning 128 x 64 (4 x 2 fragments of v_mfma_f32_32x32x16_bf16, 128 accumulator
// registers), K step 32: a stage = A_hi | A_lo | W_hi | W_lo, 256 rows x 64 B each = 64 KB, double buffered (128 of the 160 KB);
// every plane goes global -> LDS with global_load_lds_dwordx4 (no VGPR staging, no ds_write); the LDS image is lane-linear, so the
// 16-byte chunk c of row r holds the row's chunk c ^ ((r >> 2) & 3) (pre-swizzled SOURCE address, the same involution on the read
// side): ds_read_b128 fragment reads are bank-conflict free in the four 16-lane service groups of scratch/lds_bank_model.py;
// 48 MFMAs per wave between two barriers (the bf16 256 x 256 kernel has 32).  Row tiles of one column tile share an XCD's L2.
// Epilogue per wave through a private LDS region: bias (folded into the accumulator start), residual PAIR, exact GELU / GELU with the
// pre-activation kept / GELU' of a kept pre-activation, then either hi = bf16(v), lo = bf16(v - hi) as two coalesced 16-byte
// stores or fp32.  Rows may be re-based per image on either side (the class-token slot of ViT's patch embedding) and the problem
// may be batched over blockIdx.y with operand planes anywhere in memory (attention products: the "weights" are K / V activations).
// CONV instances gather the A planes on the fly like rart_conv_igemm_bf16 does (row m = (image, oy, ox) of a row grid, k = tap * k_per_tap
// + c, source pixel (oy sy + dy[tap], ox sx + dx[tap]), the zero page outside the image) -- every convolution of the reference-precision
// ResNet-50 (forward taps, flipped taps, the parity classes of a stride-2 backward, the stem's row taps) -- with 1-bit ReLU masks and
// sign bits in the epilogue; column tiles of 64 / 128 / 256 so that the 64- and 128-channel layers do not pad their MFMA work.
#include "rart_common.h"
#include <stdlib.h>

#include "rart_gemm_pair_dev.h"
#include "rart_lds_dma.h"

namespace {
// TM x TN: the tile (rows 256 / 128, columns 256 / 128 / 64), TM / 32 waves (8 / 4) in a (NW / WN) x WN grid, WN = TN / 64; a wave owns
// (TM / WM) rows x 64 columns.  The 256-row tiles are for the K-deep, MFMA-bound products (one workgroup per CU, 48 MFMAs per wave between
// two barriers at TN = 256); the 128-row tiles (48-96 KB of LDS: two or three workgroups per CU whose load / multiply / store phases
// overlap) for the short-K, HBM-bound 1x1 layers and the small-M layers of ResNet-50 whose 256-row tiling would not fill 256 CUs.
// SRC2 (CONV only): a second A source -- one tap at offset 0, a pixel geometry of its own -- feeds the K steps from d.kt1 on: a projection
// shortcut accumulated in the launch of the 1x1 it is added to.  The weight table's rows hold both sources' columns side by side, so the W
// loader walks on unchanged; the A loader picks the lane offset / resource pair by a wave-uniform compare on the step index.
// CLS (CONV + SRC2 instances): blockIdx.y selects a CLASS of the launch (d.cls): its taps, its slice of the weight rows, its K length and
// its destination parity -- the input-parity classes of a stride-2 backward in one grid.  A tile's class is block-uniform, so the K loop,
// the loader's scalar offsets and the epilogue are the single-class ones; a class whose kt1 == KT never reads the second source.
template <int TM, int TN, bool CONV, bool SRC2 = false, bool CLS = false>
__global__ __launch_bounds__(TM * 2, 1) void k_gemm_pair(const GemmPairDev d) {
  static_assert(CONV || !SRC2, "the second source is served by the conv instances");
  static_assert(!CLS || (CONV && SRC2), "classes are served by the two-source conv instances");
  const int ci = CLS ? (int)blockIdx.y : 0;
  const int tap_b = CLS ? d.cls[ci].tap_begin : 0, ntap = CLS ? d.cls[ci].n_taps : d.n_taps;
  constexpr int NW = TM / 32;
  constexpr int WN = (TN / 64 < NW) ? TN / 64 : NW, WM = NW / WN, RW = TM / WM, MI = RW / 32, NJ = TN / (32 * WN);
  static_assert(NJ == 2, "a wave owns 64 columns");
  constexpr int GP_PLANE_A = TM * GP_BK * 2;                        // one A plane of a stage: TM rows x 64 B
  constexpr int PLANE_B = TN * GP_BK * 2, STAGE = 2 * GP_PLANE_A + 2 * PLANE_B;
  constexpr int A_PIECES = TM / 16, AQ = A_PIECES / NW;             // 1 KiB pieces (16 rows x 64 B) of an A plane; per wave (2)
  constexpr int B_PIECES = TN / 16, BQ = (B_PIECES + NW - 1) / NW;  // ... of a W plane
  constexpr int GP_STAGING = NW * 32 * GP_LDE * 4;                  // NW waves x 32 rows of the epilogue transposition
  static_assert(AQ == 2, "two A pieces per wave");
  static_assert(GP_STAGING + TM * 4 <= 2 * STAGE, "epilogue staging + row table must fit the tile buffers");
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave / WN, wn = wave % WN;
  // batched problems: block-uniform base shifts (element offsets)
  const uint16_t *a_hi = d.a_hi, *a_lo = d.a_lo, *w_hi = d.w_hi, *w_lo = d.w_lo;
  long long c_off = 0;
  if (!CONV && gridDim.y > 1) {
    const int z = blockIdx.y, zo = z / d.z_inner, zi = z - zo * d.z_inner;
    const long long ao = zo * d.a_zo + zi * d.a_zi, wo = zo * d.w_zo + zi * d.w_zi;
    a_hi += ao; a_lo += ao; w_hi += wo; w_lo += wo;
    c_off = zo * d.c_zo + zi * d.c_zi;
  }
  const int TMV = d.tile_rows;                    // TM, or TM - 32 (round 6): a tile steps TMV rows, its last 32-row block is left out
  const int n_tiles = (d.N + TN - 1) / TN, m_tiles = (d.M + TMV - 1) / TMV;
  int m_tile, n_tile;
  if (m_tiles >= 16) {
    // all column tiles of a row tile on one XCD (the A tile is re-read from its L2)
    const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3;
    m_tile = (slot / n_tiles) * 8 + xcd;
    n_tile = slot % n_tiles;
    if (m_tile >= m_tiles) return;
  } else {
    m_tile = blockIdx.x / n_tiles;
    n_tile = blockIdx.x - m_tile * n_tiles;
  }
  const int m0 = m_tile * TMV, n0 = n_tile * TN;

  // ---- loader: a plane goes to LDS in 1 KiB pieces (16 rows x 64 B); wave w brings pieces w and w + 8; lane -> row (lane >> 2),
  //      LDS chunk (lane & 3) <- the row's chunk (lane & 3) ^ ((row >> 2) & 3).
  //      Round 6 (rart_lds_dma.h): the loads are buffer_load ... lds -- a lane's byte offset inside its plane is ONE constant (avoff /
  //      wvoff; RART_DMA_OOR for rows past M / past the table: the resource's range check zero-fills them, no zero page), the K step and
  //      the tap move the SCALAR offset; with taps the resource base is shifted down by the most negative tap offset and a pixel
  //      outside the image for tap t (bit t of `nok`) gets its offset ORed with RART_DMA_OOR: two vector instructions per piece and
  //      step where round 5's form had ~15 (which competed with the co-resident workgroups' MFMAs for the vector issue).
  uint32_t avoff[2], nok[2] = {0u, 0u};
  int tapreg = 0, tap_min = 0;
  const bool one_tap = !CONV || ntap == 1;
  if (CONV) {
    for (int t = 0; t < ntap; ++t) tap_min = min(tap_min, (d.tap_dy[tap_b + t] * d.src_w + d.tap_dx[tap_b + t]) * d.lda * 2);
    if (lane < ntap) tapreg = (d.tap_dy[tap_b + lane] * d.src_w + d.tap_dx[tap_b + lane]) * d.lda * 2 - tap_min;
  }
  const uint32_t tap0 = CONV ? (uint32_t)__builtin_amdgcn_readfirstlane((d.tap_dy[tap_b] * d.src_w + d.tap_dx[tap_b]) * d.lda * 2 - tap_min) : 0u;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = 16 * (wave + NW * q) + (lane >> 2);
    const int csrc = (lane & 3) ^ ((r >> 2) & 3);
    const int m = m0 + r;
    const bool ok = m < d.M;
    if (CONV) {
      const uint32_t mm = ok ? (uint32_t)m : 0u;
      const uint32_t t = gp_fastdiv(mm, d.gw_magic, d.gw_shift);
      const int ox = (int)(mm - t * (uint32_t)d.grid_w);
      const int n = (int)gp_fastdiv(t, d.gh_magic, d.gh_shift);
      const int oy = (int)(t - (uint32_t)n * (uint32_t)d.grid_h);
      const int by = oy * d.sy, bx = ox * d.sx;
      avoff[q] = (uint32_t)((n * d.src_h * d.src_w + by * d.src_w + bx) * d.lda * 2 + csrc * 16);
      for (int t2 = 0; t2 < ntap; ++t2) {
        const int iy = by + d.tap_dy[tap_b + t2], ix = bx + d.tap_dx[tap_b + t2];
        if (!(ok && (unsigned)iy < (unsigned)d.src_h && (unsigned)ix < (unsigned)d.src_w)) nok[q] |= 1u << t2;
      }
      if (one_tap && (nok[q] & 1u)) avoff[q] = RART_DMA_OOR;
    } else {
      long long srow = m;
      if (d.map_rows) {
        const int img = m / d.rpi;
        srow = (long long)img * d.src_rpi + (m - img * d.rpi);
      }
      avoff[q] = ok ? (uint32_t)(((srow + d.src_off) * d.lda + csrc * 8) * 2) : RART_DMA_OOR;
    }
  }
  uint32_t avoff2[2] = {RART_DMA_OOR, RART_DMA_OOR};
  if (SRC2) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int r = 16 * (wave + NW * q) + (lane >> 2);
      const int csrc = (lane & 3) ^ ((r >> 2) & 3);
      const int m = m0 + r;
      if (m < d.M) {      // (the host checked that every row's pixel lies inside the second source's image)
        const uint32_t t = gp_fastdiv((uint32_t)m, d.gw_magic, d.gw_shift);
        const int ox = (int)((uint32_t)m - t * (uint32_t)d.grid_w);
        const int n = (int)gp_fastdiv(t, d.gh_magic, d.gh_shift);
        const int oy = (int)(t - (uint32_t)n * (uint32_t)d.grid_h);
        avoff2[q] = (uint32_t)(((n * d.src2_h + oy * d.sy2) * d.src2_w + ox * d.sx2) * d.lda2 * 2 + csrc * 16);
      }
    }
  }
  uint32_t wvoff[BQ];
#pragma unroll
  for (int q = 0; q < BQ; ++q) {
    const int r = 16 * (wave + NW * q) + (lane >> 2);
    const int csrc = (lane & 3) ^ ((r >> 2) & 3);
    const int n = n0 + r;
    wvoff[q] = (r < TN && n < d.w_rows) ? (uint32_t)((n * d.ldw + csrc * 8) * 2) : RART_DMA_OOR;
  }
  const rart_srd_t srd_ah = rart_dma_srd(reinterpret_cast<const char*>(a_hi) + tap_min), srd_al = rart_dma_srd(reinterpret_cast<const char*>(a_lo) + tap_min);
  const rart_srd_t srd_wh = rart_dma_srd(w_hi), srd_wl = rart_dma_srd(w_lo);
  const rart_srd_t srd_a2h = rart_dma_srd(SRC2 ? d.a2_hi : a_hi), srd_a2l = rart_dma_srd(SRC2 ? d.a2_lo : a_lo);
  const int kt1 = CLS ? d.cls[ci].kt1 : (SRC2 ? d.kt1 : 0);
  const uint32_t w_off = CLS ? (uint32_t)d.cls[ci].w_off : 0u;       // (bytes) the class's slice of the weight rows
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)lds;
  // GP_W_INTERLEAVED: the weight table holds, per row and K step, the 64 bytes of the hi plane followed by the 64 bytes of the lo plane
  // (one 128-byte line per row and step; w_lo = w_hi + 32 elements) instead of two planes K apart
  const int w_step = (d.flags & GP_W_INTERLEAVED) ? 128 : 64;
#define RART_GP_ISSUE(KT, BUF)                                                                                  \
  {                                                                                                             \
    const uint32_t st_ = lds_base + (BUF)*STAGE;                                                                \
    const int kt_ = (KT);                                                                                       \
    if (SRC2 && kt_ >= kt1) {                                                                                   \
      const uint32_t so_ = (uint32_t)(kt_ - kt1) * 64u;                                                         \
      _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                           \
        rart_dma_load16(avoff2[q], srd_a2h, so_, st_ + (wave + NW * q) * 1024);                                 \
        rart_dma_load16(avoff2[q], srd_a2l, so_, st_ + GP_PLANE_A + (wave + NW * q) * 1024);                    \
      }                                                                                                         \
    } else if (one_tap) {                                                                                       \
      const uint32_t so_ = tap0 + (uint32_t)kt_ * 64u;                                                          \
      _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                           \
        rart_dma_load16(avoff[q], srd_ah, so_, st_ + (wave + NW * q) * 1024);                                   \
        rart_dma_load16(avoff[q], srd_al, so_, st_ + GP_PLANE_A + (wave + NW * q) * 1024);                      \
      }                                                                                                         \
    } else {                                                                                                    \
      const int tap_ = kt_ >> d.tpt_shift;                                                                      \
      const uint32_t so_ = (uint32_t)(__builtin_amdgcn_readlane(tapreg, tap_) + (kt_ - (tap_ << d.tpt_shift)) * 64); \
      _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                           \
        const uint32_t vo_ = avoff[q] | ((uint32_t)__builtin_amdgcn_sbfe(nok[q], tap_, 1) & RART_DMA_OOR);      \
        rart_dma_load16(vo_, srd_ah, so_, st_ + (wave + NW * q) * 1024);                                        \
        rart_dma_load16(vo_, srd_al, so_, st_ + GP_PLANE_A + (wave + NW * q) * 1024);                           \
      }                                                                                                         \
    }                                                                                                           \
    {                                                                                                           \
      const uint32_t so_ = w_off + (uint32_t)(kt_ * w_step);                                                    \
      _Pragma("unroll") for (int q = 0; q < BQ; ++q) {                                                          \
        if (NW * q + NW <= B_PIECES || wave + NW * q < B_PIECES) {   /* (first half: compile time, no branch) */  \
          rart_dma_load16(wvoff[q], srd_wh, so_, st_ + 2 * GP_PLANE_A + (wave + NW * q) * 1024);                \
          rart_dma_load16(wvoff[q], srd_wl, so_, st_ + 2 * GP_PLANE_A + PLANE_B + (wave + NW * q) * 1024);      \
        }                                                                                                       \
      }                                                                                                         \
    }                                                                                                           \
  }
  const int fr = lane & 31, h = lane >> 5;
  uint32_t xo[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) xo[ks] = (uint32_t)(fr * 64 + (((2 * ks + h) ^ ((fr >> 2) & 3)) << 4));
  // accumulators start at the bias of their column (lane & 31 is the column of a 32 x 32 MFMA tile)
  f32x16 acc[MI][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int bc = n0 + wn * 64 + j * 32 + fr;
    const float bv = (d.bias && bc < d.N) ? d.bias[bc] : 0.f;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = bv;
  }
  const int KT = CLS ? d.cls[ci].KT : d.K / GP_BK;
  const bool skip_last = wm * RW + MI * 32 > TMV;      // (wave-uniform) this wave's last row block lies past the tile's rows
  RART_GP_ISSUE(0, 0)
  rart_dma_wait<0>();
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < KT) RART_GP_ISSUE(kt + 1, buf ^ 1)
    const uint8_t* Ah = lds + buf * STAGE + (wm * RW) * 64;
    const uint8_t* Bh = lds + buf * STAGE + 2 * GP_PLANE_A + (wn * 64) * 64;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 ah[MI], al[MI], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        if (i == MI - 1 && skip_last) continue;
        ah[i] = *reinterpret_cast<const bf16x8*>(Ah + i * 32 * 64 + xo[ks]);
        al[i] = *reinterpret_cast<const bf16x8*>(Ah + GP_PLANE_A + i * 32 * 64 + xo[ks]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        bh[j] = *reinterpret_cast<const bf16x8*>(Bh + j * 32 * 64 + xo[ks]);
        bl[j] = *reinterpret_cast<const bf16x8*>(Bh + PLANE_B + j * 32 * 64 + xo[ks]);
      }
      // the two small products first, the large one last: all three land in the same fp32 accumulator
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (i == MI - 1 && skip_last) continue;
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
    rart_dma_wait<0>();                     // the next stage has landed in LDS
    __syncthreads();
  }
#undef RART_GP_ISSUE
  gp_epilogue<TM, TN, CONV, MI>(d, lds, acc, m0, n0, c_off, TMV, CLS ? d.cls[ci].dst_oy : d.dst_oy, CLS ? d.cls[ci].dst_ox : d.dst_ox);
}

// 1 (default): the 256-row tiles with 128 / 256 columns run the ping-pong schedule of csrc/gemm_pair_pp.hip; 2 (opt-in, measured slower): as 1,
// and one-tap problems with at least two 256 x 128 tiles per CU on the PERSISTENT kernel with the deferred epilogue; 0: this file's two-stage loop everywhere (the
// A/B switch of tests/test_engine_x3_gpu.py and scratch/r6/).  Bit-identical outputs under all three.  RART_PAIR_SCHEDULE in the environment
// sets the initial value.
int g_pair_schedule = -1;
long long gp_env(const char* name, long long unset) {
  const char* e = getenv(name);
  return e ? atoll(e) : unset;
}
int gp_schedule() {
  if (g_pair_schedule < 0) g_pair_schedule = (int)gp_env("RART_PAIR_SCHEDULE", 1);
  return g_pair_schedule;
}

// The schedule and the lab switches of one call.  The environment is read here and nowhere else, once per variable and on EVERY call: the
// tests flip RART_PAIR_ROWS224 / RART_PAIR_SPLIT inside one process.
struct GpLab {
  int schedule;             // above
  int rows224;              // RART_PAIR_ROWS224: tiles that leave their last 32-row block out (default 1: the ping-pong kernel's 224-row tiles; 2 / 3: the two-stage kernel's too, 3 for K >= 1024 only)
  int split;                // RART_PAIR_SPLIT: the remainder split (default on)
  long long nt_min_mb;      // RART_PAIR_NT_MIN_MB: non-temporal epilogue streams for output pairs of at least this size (default 0: all)
};
GpLab gp_read_lab() {
  return GpLab{gp_schedule(), (int)gp_env("RART_PAIR_ROWS224", 1), (int)gp_env("RART_PAIR_SPLIT", 1), gp_env("RART_PAIR_NT_MIN_MB", 0)};
}

void gp_magic(uint32_t dv, uint32_t& mg, uint32_t& sh) {   // exact for dividends < 2^31
  uint32_t l = 0;
  while ((1ull << l) < dv) ++l;
  sh = 31 + l;
  mg = (uint32_t)(((1ull << sh) + dv - 1) / dv);
}
}  // namespace

bool rart_gemm_pair_pp_has(int tn, bool conv, bool src2, bool cls, bool walk);   // gemm_pair_pp.hip
bool rart_gemm_pair_pp_launch(const void* dev_desc, int tn, bool conv, unsigned grid_x, unsigned grid_y, hipStream_t st, unsigned walk_wgs);
void rart_gemm_pair_ps_launch(const void* dev_desc, bool conv, unsigned wgs, hipStream_t st);

namespace {
int gp_cu_count() {      // compute units of the current device (the persistent kernel's grid), per device
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int n = 0;
    cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
  }
  return cus[dev];
}
}  // namespace

extern "C" int rart_gemm_pair_set_schedule(int mode) {
  RART_CHECK_ARG(mode >= 0 && mode <= 3,
                 "rart_gemm_pair_set_schedule: mode must be 0 (two-stage loop), 1 (ping-pong), 2 (ping-pong + deferred-epilogue persistent) or 3 (ping-pong, tiles walked)");
  g_pair_schedule = mode;
  return RART_OK;
}
extern "C" int rart_gemm_pair_get_schedule(void) { return gp_schedule(); }

// Tile policy, from the per-shape sweep of every launch of a ResNet-50 gradient evaluation at B = 256 (scratch/r4/sweep_pair_tiles.py,
// profiles/r04_pair_tile_sweep.txt).  Plain products (the transformer GEMMs): 256 rows x the widest of 64 / 128 / 256 columns that does not
// pad the MFMA work.  Convolutions: K <= 256 (the HBM-bound 1x1 layers: two K steps do not hide a tile's load and store phases) 256 x 64,
// 80 KB of LDS = two workgroups per CU; K < 1024 128 x {128, 64} (64 / 48 KB: two or three per CU); K-deep wide layers 256 x 256 unless
// that leaves fewer than 128 workgroups (layer4: 256 x 128), K-deep narrow layers (N <= 128) 128 x N.  tile_m / tile_n override.
// Two-source launches (a projection shortcut folded into its 1x1: K = K1 + K2) take the same policy; swept at B = 256
// (profiles/shortcut_fusion_tile_sweep.txt, us per launch, chosen tile first): 200704 x 384 -> 512: 308 on 224-row x 256 ping-pong (256 x 256
// 319, 128 x 128 349, 256 x 64 386); 50176 x 768 -> 1024: 259 on 224 x 256 (256 x 256 273, 128 x 128 289); 12544 x 1536 -> 2048: 206 on
// 224 x 256 (256 x 256 214, 256 x 128 258); layer1's backward 802816 x 320 -> 64: 246 on 128 x 64 (256 x 64 252).
// A class launch (ncls > 1 grids of the same tiles) counts its workgroups over all classes.
static void gp_tile_policy(bool conv, int M, int N, int K, int schedule, int& tm, int& tn, int ncls = 1) {
  tn = N <= 64 ? 64 : (N <= 128 ? 128 : 256);
  tm = 256;
  if (conv) {
    if (schedule >= 1 && N >= 256 && (K >= 512 || (K >= 256 && N <= 512))) {
      // round 6 (scratch/r6/time_pair_pp.py --tiles, profiles/r06_pair_pp.json): with the ping-pong schedule the 256-row tiles win wherever
      // the layer is at least 256 wide and 256 deep -- 256 x 256 unless that leaves fewer than 128 workgroups (layer4: 256 x 128); the one
      // exception measured: K = 256 into >= 1024 columns (layer3's expansion: epilogue-bound, 155-165 us on 256 x 64 vs 166-176).  128-column
      // layers (layer2's 3 x 3 once its tail kernel is off) stay on the two-stage 128 x 128 tiles: 19.97 vs 20.14 ms on 256 x 128 ping-pong
      tm = 256;
      tn = (long long)((M + 255) / 256) * ((N + 255) / 256) * ncls < 128 ? 128 : 256;
    } else if (K <= 256) { tm = 256; tn = 64; }
    else if (K < 1024 || N <= 128) { tm = 128; tn = N <= 64 ? 64 : 128; }
    else if ((long long)((M + 255) / 256) * ((N + 255) / 256) * ncls < 128) { tm = 256; tn = 128; }
    if (M <= 256) { tm = 128; tn = 64; }
  }
}

// A checked problem: the device descriptor and what the caller's descriptor says beside it.  A second source shows as d.a2_hi, a class
// table as d.n_cls > 0.
struct GpProblem {
  GemmPairDev d;
  bool conv;
  int nz;                   // batched problems (blockIdx.y of a launch without classes)
  int tile_m, tile_n;       // the caller's overrides (0: the tile policy's choice)
};

// Step 1 of gp_launch: the argument checks and the device descriptor, complete but for what a launch record sets (M, m_begin, tile_rows:
// here the whole problem on full 256-row tiles).  s2 / cd: see gp_launch.
static int gp_check_and_fill(const rart_gemm_pair_desc* h, const rart_gemm_pair2_desc* s2, const rart_gemm_pair_cls_desc* cd, const GpLab& lab,
                             GpProblem& p) {
  RART_CHECK_ARG(h != nullptr, "rart_gemm_pair_bf16: null descriptor");
  RART_CHECK_ARG(h->a_hi && h->a_lo && h->w_hi && h->w_lo && h->dst_hi, "rart_gemm_pair_bf16: null operand plane");
  const bool conv = h->conv != 0;
  GemmPairDev& d = p.d;
  d = GemmPairDev{};
  d.M = h->M; d.K = h->K;
  const bool src2 = s2 != nullptr;
  RART_CHECK_ARG(!src2 || (conv && s2->a2_hi && s2->a2_lo), "rart_gemm_pair2_bf16: the second source is a pair (both planes) and is served by conv mode only");
  if (conv) {
    RART_CHECK_ARG(h->batch > 0 && h->grid_h > 0 && h->grid_w > 0 && h->src_h > 0 && h->src_w > 0 && h->dst_h > 0 && h->dst_w > 0,
                   "rart_gemm_pair_bf16 (conv): empty geometry");
    RART_CHECK_ARG(h->n_taps >= 1 && h->n_taps <= 16, "rart_gemm_pair_bf16 (conv): n_taps must be 1..16");
    RART_CHECK_ARG(h->k_per_tap >= 32 && (h->k_per_tap & (h->k_per_tap - 1)) == 0,
                   "rart_gemm_pair_bf16 (conv): k_per_tap must be a power of two >= 32");
    RART_CHECK_ARG(h->n_batched <= 1 && h->rows_per_image == 0 && h->src_row_off == 0 && h->dst_row_off == 0,
                   "rart_gemm_pair_bf16 (conv): no batching / row re-basing in conv mode");
    const long long M = (long long)h->batch * h->grid_h * h->grid_w;
    RART_CHECK_ARG(M < (1ll << 31), "rart_gemm_pair_bf16 (conv): row grid must stay below 2^31 rows");
    RART_CHECK_ARG((long long)h->batch * h->src_h * h->src_w * h->lda < (1ll << 30) && (long long)h->batch * h->dst_h * h->dst_w * h->ldc < (1ll << 31),
                   "rart_gemm_pair_bf16 (conv): a source plane must stay below 2 GiB (32-bit byte offsets of the stage loads) and the destination "
                   "below 2^31 elements (split the batch)");
    RART_CHECK_ARG(h->lda % 8 == 0 || h->lda == 4, "rart_gemm_pair_bf16 (conv): source pixels must keep 16-byte alignment of the K chunks");
    // (the conv instances are compiled without the GELU forms: gp_finish_segment<true, false>)
    RART_CHECK_ARG(!(h->flags & (GP_GELU | GP_GELU_BWD | GP_GELU_KEEP)), "rart_gemm_pair_bf16 (conv): the GELU forms are served by plain products only");
    d.M = (int)M;
    d.K = h->k_per_tap * h->n_taps;
    if (src2) {
      RART_CHECK_ARG(s2->k2 >= 32 && s2->k2 % GP_BK == 0, "rart_gemm_pair2_bf16: k2 must be a positive multiple of 32");
      RART_CHECK_ARG(s2->lda2 % 8 == 0 && s2->lda2 >= s2->k2, "rart_gemm_pair2_bf16: lda2 must cover k2 and keep 16-byte alignment of the K chunks");
      RART_CHECK_ARG(s2->src2_h > 0 && s2->src2_w > 0 && s2->sy2 > 0 && s2->sx2 > 0 && (long long)(h->grid_h - 1) * s2->sy2 < s2->src2_h &&
                         (long long)(h->grid_w - 1) * s2->sx2 < s2->src2_w,
                     "rart_gemm_pair2_bf16: every row's pixel must lie inside the second source's image");
      RART_CHECK_ARG((long long)h->batch * s2->src2_h * s2->src2_w * s2->lda2 < (1ll << 30),
                     "rart_gemm_pair2_bf16: the second source plane must stay below 2 GiB (split the batch)");
      d.a2_hi = (const uint16_t*)s2->a2_hi; d.a2_lo = (const uint16_t*)s2->a2_lo;
      d.lda2 = s2->lda2; d.kt1 = d.K / GP_BK; d.src2_h = s2->src2_h; d.src2_w = s2->src2_w; d.sy2 = s2->sy2; d.sx2 = s2->sx2;
      d.K += s2->k2;
    }
    d.grid_h = h->grid_h; d.grid_w = h->grid_w; d.src_h = h->src_h; d.src_w = h->src_w; d.sy = h->sy; d.sx = h->sx; d.n_taps = h->n_taps;
    int sh = 0;
    while ((32 << sh) < h->k_per_tap) ++sh;
    d.tpt_shift = sh;
    for (int i = 0; i < 16; ++i) { d.tap_dy[i] = i < h->n_taps ? h->tap_dy[i] : 0; d.tap_dx[i] = i < h->n_taps ? h->tap_dx[i] : 0; }
    d.dst_h = h->dst_h; d.dst_w = h->dst_w; d.dst_sy = h->dst_sy; d.dst_sx = h->dst_sx; d.dst_oy = h->dst_oy; d.dst_ox = h->dst_ox;
    gp_magic((uint32_t)d.grid_w, d.gw_magic, d.gw_shift);
    gp_magic((uint32_t)d.grid_h, d.gh_magic, d.gh_shift);
    d.mask_bits = (const uint8_t*)h->mask_bits; d.sign_out = (uint8_t*)h->sign_out;
    RART_CHECK_ARG(!(d.sign_out && (h->flags & GP_OUT_F32)), "rart_gemm_pair_bf16 (conv): sign_out needs a pair destination");
    if (cd) {
      // the class table, longest K first (the dispatcher hands out blockIdx.y = 0 first); d.K = the longest, which the tile policy reads
      const int n = cd->n_classes, k2 = src2 ? s2->k2 : 0;
      int order[4] = {0, 1, 2, 3};
      auto klen = [&](int i) { return h->k_per_tap * cd->cls[i].n_taps + (cd->cls[i].src2 ? k2 : 0); };
      for (int i = 1; i < n; ++i)
        for (int j = i; j > 0 && klen(order[j]) > klen(order[j - 1]); --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
      d.n_cls = n;
      for (int i = 0; i < n; ++i) {
        const rart_gemm_pair_class& c = cd->cls[order[i]];
        d.cls[i].tap_begin = c.tap_begin; d.cls[i].n_taps = c.n_taps; d.cls[i].w_off = c.k_off * 2;
        d.cls[i].kt1 = h->k_per_tap * c.n_taps / GP_BK; d.cls[i].KT = klen(order[i]) / GP_BK;
        d.cls[i].dst_oy = c.dst_oy; d.cls[i].dst_ox = c.dst_ox; d.cls[i].pad_ = 0;
      }
      d.K = klen(order[0]);
    }
  } else {
    RART_CHECK_ARG(!h->mask_bits && !h->sign_out, "rart_gemm_pair_bf16: mask_bits / sign_out are served by conv mode only");
    RART_CHECK_ARG(h->lda % 8 == 0 && h->lda >= h->K, "rart_gemm_pair_bf16: lda must cover the row and keep 16-byte alignment");
    d.grid_h = d.grid_w = d.src_h = d.src_w = d.sy = d.sx = d.n_taps = 1; d.tpt_shift = 0;
    for (int i = 0; i < 16; ++i) d.tap_dy[i] = d.tap_dx[i] = 0;
    d.dst_h = d.dst_w = d.dst_sy = d.dst_sx = 1; d.dst_oy = d.dst_ox = 0;
    d.gw_magic = d.gw_shift = d.gh_magic = d.gh_shift = 0;
    d.mask_bits = nullptr; d.sign_out = nullptr;
  }
  d.N = h->N;
  RART_CHECK_ARG(d.M > 0 && d.N > 0 && d.N % 8 == 0, "rart_gemm_pair_bf16: M > 0, N a positive multiple of 8");
  RART_CHECK_ARG(d.K > 0 && d.K % GP_BK == 0, "rart_gemm_pair_bf16: K must be a positive multiple of 32");
  RART_CHECK_ARG(h->ldw % 8 == 0 && h->ldc % 8 == 0 && h->ldw >= d.K && h->ldc >= d.N,
                 "rart_gemm_pair_bf16: leading dimensions must cover the row and keep 16-byte alignment");
  RART_CHECK_ARG((long long)(h->w_rows > 0 ? h->w_rows : h->N) * h->ldw < (1ll << 30), "rart_gemm_pair_bf16: a weight plane must stay below 2 GiB");
  if (!conv) {
    const long long imgs = (h->rows_per_image > 0 && h->rows_per_image < d.M) ? (d.M + h->rows_per_image - 1) / h->rows_per_image : 1;
    const long long src_rows = imgs > 1 ? imgs * (h->src_rows_per_image > 0 ? h->src_rows_per_image : h->rows_per_image) : d.M;
    RART_CHECK_ARG((src_rows + h->src_row_off) * h->lda < (1ll << 30), "rart_gemm_pair_bf16: a source plane must stay below 2 GiB (per batched problem)");
  }
  const bool out_f32 = (h->flags & GP_OUT_F32) != 0;
  RART_CHECK_ARG(out_f32 || h->dst_lo, "rart_gemm_pair_bf16: a pair destination needs its lo plane");
  RART_CHECK_ARG((h->res_hi == nullptr) == (h->res_lo == nullptr), "rart_gemm_pair_bf16: the residual is a pair: both planes or none");
  RART_CHECK_ARG(!(h->flags & (GP_GELU_KEEP | GP_GELU_BWD)) || (h->aux_hi && h->aux_lo),
                 "rart_gemm_pair_bf16: GELU_KEEP / GELU_BWD need the pre-activation pair (aux)");
  RART_CHECK_ARG(!(h->flags & ~(GP_OUT_F32 | GP_GELU | GP_GELU_BWD | GP_GELU_KEEP | GP_RELU | GP_W_INTERLEAVED)), "rart_gemm_pair_bf16: unknown flag");
  RART_CHECK_ARG(!(h->flags & GP_W_INTERLEAVED) || h->ldw >= 2 * d.K, "rart_gemm_pair_bf16: an interleaved weight table has rows of 2 K elements");
  {
    const int g = (h->flags & GP_GELU ? 1 : 0) + (h->flags & GP_GELU_BWD ? 1 : 0) + (h->flags & GP_GELU_KEEP ? 1 : 0);
    RART_CHECK_ARG(g <= 1 && !((h->flags & GP_GELU_KEEP) && out_f32), "rart_gemm_pair_bf16: at most one GELU mode; GELU_KEEP writes pairs");
  }
  d.a_hi = (const uint16_t*)h->a_hi; d.a_lo = (const uint16_t*)h->a_lo; d.w_hi = (const uint16_t*)h->w_hi; d.w_lo = (const uint16_t*)h->w_lo;
  d.bias = h->bias; d.res_hi = (const uint16_t*)h->res_hi; d.res_lo = (const uint16_t*)h->res_lo;
  d.dst_hi = (uint16_t*)h->dst_hi; d.dst_lo = (uint16_t*)h->dst_lo; d.aux_hi = (uint16_t*)h->aux_hi; d.aux_lo = (uint16_t*)h->aux_lo;
  d.lda = h->lda; d.ldw = h->ldw; d.ldc = h->ldc;
  d.w_rows = h->w_rows > 0 ? h->w_rows : h->N;
  d.map_rows = (!conv && h->rows_per_image > 0 && h->rows_per_image < d.M) ? 1 : 0;
  d.rpi = d.map_rows ? h->rows_per_image : d.M;
  d.src_rpi = h->src_rows_per_image > 0 ? h->src_rows_per_image : d.rpi;
  d.dst_rpi = h->dst_rows_per_image > 0 ? h->dst_rows_per_image : d.rpi;
  d.src_off = h->src_row_off; d.dst_off = h->dst_row_off;
  RART_CHECK_ARG(d.src_off >= 0 && d.dst_off >= 0, "rart_gemm_pair_bf16: row offsets must be >= 0");
  d.flags = h->flags;
  // non-temporal epilogue streams for outputs that do not stay cached anyway (lab switch: the output pair's size)
  d.nt = (long long)d.M * d.N * 4 >= lab.nt_min_mb * (1ll << 20) ? 1 : 0;
  p.nz = h->n_batched > 1 ? h->n_batched : 1;
  RART_CHECK_ARG(p.nz <= 65535, "rart_gemm_pair_bf16: n_batched must be <= 65535");
  d.z_inner = h->z_inner > 0 ? h->z_inner : 1;
  d.a_zo = h->a_z_outer; d.a_zi = h->a_z_inner; d.w_zo = h->w_z_outer; d.w_zi = h->w_z_inner; d.c_zo = h->c_z_outer; d.c_zi = h->c_z_inner;
  d.m_begin = 0;
  d.tile_rows = 256;
  p.conv = conv; p.tile_m = h->tile_m; p.tile_n = h->tile_n;
  return RART_OK;
}

// A launch runs in passes of one tile per CU and XCD: workgroup i goes to XCD i % GP_XCDS, and from 16 row tiles on the kernels enumerate
// the row tiles in groups of GP_XCDS, XCD x taking the row tiles x, x + GP_XCDS, ... with all their column tiles (the A tile is re-read
// from that XCD's L2).
constexpr int GP_XCDS = 8;
static int gp_row_enum(int mt) { return mt >= 16 ? (mt + GP_XCDS - 1) / GP_XCDS * GP_XCDS : mt; }      // row tiles a grid enumerates
// passes of mt x nt tiles over `slots` resident workgroups per XCD
static int gp_passes(int mt, int nt, int slots) {
  if (slots < 1) slots = 1;
  return ((mt >= 16 ? (mt + GP_XCDS - 1) / GP_XCDS * nt : (mt * nt + GP_XCDS - 1) / GP_XCDS) + slots - 1) / slots;
}
// the launch of rows m_begin .. M - 1 on tm x tn tiles that step tile_rows rows
static rart_gemm_pair_launch_rec gp_record(int family, int tm, int tn, int tile_rows, int m_begin, int M, int N, unsigned grid_y) {
  const long long tiles = (long long)gp_row_enum((M - m_begin + tile_rows - 1) / tile_rows) * ((N + tn - 1) / tn);
  return rart_gemm_pair_launch_rec{family, tm, tn, tile_rows, m_begin, M, (unsigned)tiles, grid_y, 0u, family == RART_GP_TWO_STAGE ? tm * 2u : 512u};
}

// Step 2 of gp_launch: what to launch for a checked problem on a device of `cus` compute units.  A function of its arguments alone (no HIP
// call, no environment, no state); false: the grid would be too large.
static bool gp_plan(const GpProblem& p, const GpLab& lab, int cus, rart_gemm_pair_plan& plan) {
  const GemmPairDev& d = p.d;
  const bool conv = p.conv, src2 = d.a2_hi != nullptr, cls = d.n_cls > 0, forced = p.tile_m != 0 || p.tile_n != 0;
  const int nz = p.nz, ncls = cls ? d.n_cls : 1;
  // A class launch takes the tiles of its longest class for all of them.  Measured at B = 256 (profiles/first_block_folds_per_part.txt): the
  // K = 640 + 3 x K = 128 classes of layer2's folded shortcut^T run 505 us as one 256 x 256 ping-pong grid against 560 us as two launches
  // with each class on the tiles its own K would choose (622 us before the fold).
  int tn, tm;
  gp_tile_policy(conv, d.M, d.N, d.K, lab.schedule, tm, tn, ncls);
  if (p.tile_n == 64 || p.tile_n == 128 || p.tile_n == 256) tn = p.tile_n;
  if (p.tile_m == 128 || p.tile_m == 256) tm = p.tile_m;
  if (p.tile_m == 224) tm = 256;            // the ping-pong kernel's 224-row form (below)
  const int m_tiles = (d.M + tm - 1) / tm, n_tiles = (d.N + tn - 1) / tn;
  const long long blocks = (long long)gp_row_enum(m_tiles) * n_tiles;
  if (blocks >= (1ll << 31)) return false;
  const unsigned grid_y = cls ? ncls : nz;      // a class launch: blockIdx.y = class (conv mode is unbatched: nz == 1)
  const int cx = cus / GP_XCDS;                 // CUs per XCD
  const bool pp_tiles = tm == 256 && tn >= 128 && lab.schedule >= 1;      // the tiles the ping-pong kernel has
  plan = rart_gemm_pair_plan{};
  plan.n_launches = 1;
  rart_gemm_pair_launch_rec& r = plan.launch[0];
  // the persistent kernel (256 x 128 tiles, deferred epilogue): one tap, no GELU epilogue, no row re-basing / batching, at least two tiles per
  // CU and a K loop with room for the 12 micro-steps of a tile's epilogue
  if (lab.schedule == 2 && !src2 && !cls && pp_tiles && !forced && nz == 1 && !d.map_rows && d.src_off == 0 && (!conv || d.n_taps == 1) &&
      !(d.flags & (GP_GELU | GP_GELU_BWD | GP_GELU_KEEP)) && d.K / GP_BK >= 6 && (long long)((d.M + 255) / 256) * ((d.N + 127) / 128) >= 2ll * cus) {
    r = rart_gemm_pair_launch_rec{RART_GP_PERSISTENT, 256, 128, 256, 0, d.M, (unsigned)cus, 1u, (unsigned)cus, 512u};      // one workgroup per CU
    return true;
  }
  if (pp_tiles && nz == 1 && (p.tile_m == 224 || (p.tile_m == 0 && lab.rows224)) && rart_gemm_pair_pp_has(tn, conv, src2, cls, false)) {
    // Round 6: 224-row tiles.  ResNet-50's 50176 / 12544 rows are 196 / 49 tiles of 256 rows = 25 / 7 of an XCD's 32 CUs in the fullest
    // XCD.  A tile that steps 224 rows (the kernel leaves its last 32-row block out; loads, waits and barriers unchanged) makes 224 / 56
    // row tiles = 28 / 7 per XCD: the same passes, 7/8 of the matrix work per tile.
    const int mt224 = (d.M + 223) / 224;
    // A class launch streams ncls grids of unequal K through the CUs, so whole passes mean little: what 224-row tiles can still buy is the
    // balance between the XCDs -- row tiles on the fullest one, (m_tiles + 7) / 8, against 7/8 of the work in each of (mt224 + 7) / 8 --
    // and they cost about 6 % per unit of work (more tiles for the same rows).  Measured at B = 256: 12544 rows (49 -> 56 row tiles: 7 -> 7
    // x 7/8) 171 -> 167 us (3x3) and 333 -> 317 us (shortcut^T); 50176 rows (25 -> 28 x 7/8) 180 -> 189 us; 200704 rows 505 -> 530 us.
    const bool saves = cls ? (mt224 + GP_XCDS - 1) / GP_XCDS * 0.875 * 1.06 < (m_tiles + GP_XCDS - 1) / GP_XCDS
                           : gp_passes(mt224, n_tiles, cx) * 0.92 < gp_passes(m_tiles, n_tiles, cx) - 0.01;
    if (p.tile_m == 224 || saves) {
      r = gp_record(RART_GP_PING_PONG, 256, tn, 224, 0, d.M, d.N, grid_y);
      return true;
    }
  }
  if (!conv && pp_tiles && tn == 256 && lab.split && nz == 1 && !forced && rart_gemm_pair_pp_has(256, conv, src2, cls, false) &&
      rart_gemm_pair_pp_has(128, conv, src2, cls, false)) {
    // Round 6 (scratch/r6/time_pair_rounds.py, GRBM_GUI_ACTIVE per launch): ViT-B/16's 50432 x 768 outputs (197 x 3 tiles, 75 per XCD of
    // 32 CUs) take THREE tile times for 2.3 passes of work.  Such a launch is issued as two: the row tiles of the whole passes on 256 x 256
    // tiles, the remaining rows (m_begin) on 256 x 128 tiles, which take about half a tile time.
    // Same products in the same order per output element: same bits.  Plain products only: on the convolutions of ResNet-50 (short K, epilogue-
    // heavy tiles) the second launch costs what it saves (same-box A/B 19.53 vs 19.60 ms per gradient evaluation); ViT-B/16 66.9 -> 65.9 ms.
    const double half_cost = 0.8;                          // measured: the second launch costs ~0.8 tile times (it starts when the first has drained)
    const int n128 = (d.N + 127) / 128, whole = gp_passes(m_tiles, n_tiles, cx);
    double best = whole;
    int best_ma = 0;
    for (int pa = 1; pa < whole; ++pa) {
      const int ma = pa * cx / n_tiles * GP_XCDS;          // row tiles of the first launch: pa passes exactly on every XCD
      if (ma < 16 || ma >= m_tiles) continue;
      const double c = gp_passes(ma, n_tiles, cx) + half_cost * gp_passes(m_tiles - ma, n128, cx) + 0.05;
      if (c < best - 0.1) { best = c; best_ma = ma; }
    }
    if (best_ma > 0) {
      plan.n_launches = 2;
      r = gp_record(RART_GP_PING_PONG, 256, 256, 256, 0, best_ma * 256, d.N, 1);
      plan.launch[1] = gp_record(RART_GP_PING_PONG, 256, 128, 256, best_ma * 256, d.M, d.N, 1);
      return true;
    }
  }
  // schedule 3: launches of more than one tile per CU are WALKED by one workgroup per CU (k_gemm_pair_pp, OPT bit 1)
  const unsigned walk_wgs = (lab.schedule == 3 && !src2 && !cls && nz == 1 && blocks > (long long)cus) ? (unsigned)(cus & ~(GP_XCDS - 1)) : 0u;
  if (pp_tiles && rart_gemm_pair_pp_has(tn, conv, src2, cls, walk_wgs > 0)) {
    r = gp_record(RART_GP_PING_PONG, 256, tn, 256, 0, d.M, d.N, grid_y);
    if (walk_wgs) {
      r.walk_wgs = walk_wgs;
      if (walk_wgs < r.grid_x) r.grid_x = walk_wgs;
    }
    return true;
  }
  // the two-stage kernel: tiles that step tm - 32 rows where that saves work per pass (resident workgroups per CU by LDS: 2 x STAGE bytes each)
  int rows = tm;
  if ((lab.rows224 == 2 || (lab.rows224 == 3 && d.K >= 1024)) && nz == 1 && !cls && !forced && lab.schedule >= 1) {   // (3: K-deep only)
    const int lds = 2 * (2 * tm * 64 + 2 * tn * 64), res = lds > 80 * 1024 ? 1 : (lds > 53 * 1024 ? 2 : 3);
    const int less = tm - 32, mt_less = (d.M + less - 1) / less;
    if (gp_passes(mt_less, n_tiles, cx * res) * (double)less / tm * 1.03 < gp_passes(m_tiles, n_tiles, cx * res)) rows = less;
  }
  r = gp_record(RART_GP_TWO_STAGE, tm, tn, rows, 0, d.M, d.N, grid_y);
  return true;
}

// Step 3 of gp_launch: the launches of a plan.  A record sets the descriptor's row range and tile step; nothing else differs between the
// launches of a plan.
static int gp_issue(const GpProblem& p, const rart_gemm_pair_plan& plan, rart_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  const char* what = "rart_gemm_pair_bf16";
  for (int i = 0; i < plan.n_launches; ++i) {
    const rart_gemm_pair_launch_rec& r = plan.launch[i];
    GemmPairDev d = p.d;
    d.M = r.M; d.m_begin = r.m_begin; d.tile_rows = r.tile_rows;
    const int tm = r.tile_m, tn = r.tile_n;
    if (r.family == RART_GP_PERSISTENT) {
      rart_gemm_pair_ps_launch(&d, p.conv, r.grid_x, st);
      what = "rart_gemm_pair_bf16 (persistent)";
      continue;
    }
    if (r.family == RART_GP_PING_PONG) {
      if (!rart_gemm_pair_pp_launch(&d, tn, p.conv, r.grid_x, r.grid_y, st, r.walk_wgs)) {
        rart_set_error("rart_gemm_pair_bf16: internal error: the plan chose a ping-pong instance that does not exist (%d columns)", tn);
        return RART_ERR_INVALID;
      }
      what = plan.n_launches == 2 ? "rart_gemm_pair_bf16 (ping-pong, remainder split)"
                                  : (r.tile_rows == 224 ? "rart_gemm_pair_bf16 (ping-pong, 224-row tiles)" : "rart_gemm_pair_bf16 (ping-pong)");
      continue;
    }
    const dim3 grid(r.grid_x, r.grid_y);
#define RART_GP_LAUNCH(TM_, TN_, ...) hipLaunchKernelGGL((k_gemm_pair<TM_, TN_, __VA_ARGS__>), grid, dim3(TM_ * 2), 0, st, d)
#define RART_GP_BY_TN(TM_, ...)                                            \
  do {                                                                     \
    if (tn == 64) RART_GP_LAUNCH(TM_, 64, __VA_ARGS__);                    \
    else if (tn == 128) RART_GP_LAUNCH(TM_, 128, __VA_ARGS__);             \
    else RART_GP_LAUNCH(TM_, 256, __VA_ARGS__);                            \
  } while (0)
    if (d.n_cls > 0) {
      if (tm == 128) RART_GP_BY_TN(128, true, true, true);
      else RART_GP_BY_TN(256, true, true, true);
    } else if (d.a2_hi) {
      if (tm == 128) RART_GP_BY_TN(128, true, true);
      else RART_GP_BY_TN(256, true, true);
    } else if (p.conv) {
      if (tm == 128) RART_GP_BY_TN(128, true);
      else RART_GP_BY_TN(256, true);
    } else {
      if (tm == 128) RART_GP_BY_TN(128, false);
      else RART_GP_BY_TN(256, false);
    }
#undef RART_GP_BY_TN
#undef RART_GP_LAUNCH
  }
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}

// One call of rart_gemm_pair_bf16 (s2 == nullptr), rart_gemm_pair2_bf16 (s2: the descriptor that carries the second A source) or
// rart_gemm_pair_classes_bf16 (cd: the classes of the grid, checked by that entry; s2 = the second source of the class that has src2 set):
// check, plan, issue.  plan_out: rart_gemm_pair_plan_bf16 -- the plan for `cus` compute units is returned instead of issued.
static int gp_launch(const rart_gemm_pair_desc* h, const rart_gemm_pair2_desc* s2, rart_stream_t stream, const rart_gemm_pair_cls_desc* cd,
                     rart_gemm_pair_plan* plan_out, int cus) {
  const GpLab lab = gp_read_lab();
  GpProblem p;
  if (const int bad = gp_check_and_fill(h, s2, cd, lab, p)) return bad;
  if (cus <= 0) cus = gp_cu_count();        // (after the checks: a bad descriptor is refused before any HIP call)
  rart_gemm_pair_plan plan;
  RART_CHECK_ARG(gp_plan(p, lab, cus, plan), "rart_gemm_pair_bf16: grid too large");
  if (plan_out) {
    *plan_out = plan;
    return RART_OK;
  }
  return gp_issue(p, plan, stream);
}

extern "C" int rart_gemm_pair_bf16(const rart_gemm_pair_desc* h, rart_stream_t stream) { return gp_launch(h, nullptr, stream, nullptr, nullptr, 0); }

// Two A sources (include/robustart_hip.h): the launch `one` describes, and when a2_hi is set the second source's K steps after its own.
static int gp_launch2(const rart_gemm_pair2_desc* h, rart_stream_t stream, rart_gemm_pair_plan* plan_out, int cus) {
  RART_CHECK_ARG(h != nullptr, "rart_gemm_pair2_bf16: null descriptor");
  RART_CHECK_ARG((h->a2_hi == nullptr) == (h->a2_lo == nullptr), "rart_gemm_pair2_bf16: the second source is a pair: both planes or none");
  return gp_launch(&h->one, h->a2_hi ? h : nullptr, stream, nullptr, plan_out, cus);
}
extern "C" int rart_gemm_pair2_bf16(const rart_gemm_pair2_desc* h, rart_stream_t stream) { return gp_launch2(h, stream, nullptr, 0); }
extern "C" int rart_gemm_pair_max_sources(void) { return 2; }

// Up to four classes of a conv-mode pair launch in one grid (include/robustart_hip.h): the checks, then gp_launch with the class table.
extern "C" int rart_gemm_pair_max_classes(void) { return 4; }
static int gp_launch_classes(const rart_gemm_pair_cls_desc* c, rart_stream_t stream, rart_gemm_pair_plan* plan_out, int cus) {
  RART_CHECK_ARG(c != nullptr, "rart_gemm_pair_classes_bf16: null descriptor");
  const rart_gemm_pair_desc& h = c->two.one;
  RART_CHECK_ARG(c->n_classes >= 1 && c->n_classes <= 4, "rart_gemm_pair_classes_bf16: 1..4 classes");
  RART_CHECK_ARG(h.conv != 0 && h.batch > 0 && h.grid_h > 0 && h.grid_w > 0 && h.dst_sy > 0 && h.dst_sx > 0,
                 "rart_gemm_pair_classes_bf16: classes are served by conv mode only");
  RART_CHECK_ARG(h.n_taps >= 1 && h.n_taps <= 16 && h.k_per_tap >= 32, "rart_gemm_pair_classes_bf16: 1..16 taps in all, k_per_tap >= 32");
  RART_CHECK_ARG(!(h.flags & GP_W_INTERLEAVED), "rart_gemm_pair_classes_bf16: no interleaved weight table");
  RART_CHECK_ARG((c->two.a2_hi == nullptr) == (c->two.a2_lo == nullptr), "rart_gemm_pair_classes_bf16: the second source is a pair: both planes or none");
  const bool has2 = c->two.a2_hi != nullptr;
  RART_CHECK_ARG(!has2 || (c->two.k2 >= 32 && c->two.k2 % GP_BK == 0), "rart_gemm_pair_classes_bf16: k2 must be a positive multiple of 32");
  for (int i = 0; i < c->n_classes; ++i) {
    const rart_gemm_pair_class& k = c->cls[i];
    RART_CHECK_ARG(k.tap_begin >= 0 && k.n_taps >= 1 && k.tap_begin + k.n_taps <= 16 && k.tap_begin + k.n_taps <= h.n_taps,
                   "rart_gemm_pair_classes_bf16: a class's taps must lie inside the filled tap slots (sixteen at most)");
    RART_CHECK_ARG(k.src2 == 0 || (i == 0 && has2), "rart_gemm_pair_classes_bf16: the second source rides in class 0 only, and needs its planes");
    const long long K = (long long)h.k_per_tap * k.n_taps + (k.src2 ? c->two.k2 : 0);
    RART_CHECK_ARG(k.k_off >= 0 && k.k_off % 8 == 0 && k.k_off + K <= h.ldw,
                   "rart_gemm_pair_classes_bf16: a class's slice must lie inside the rows of the weight table and keep 16-byte alignment");
    RART_CHECK_ARG(k.dst_oy >= 0 && k.dst_ox >= 0 && (long long)(h.grid_h - 1) * h.dst_sy + k.dst_oy < h.dst_h &&
                       (long long)(h.grid_w - 1) * h.dst_sx + k.dst_ox < h.dst_w,
                   "rart_gemm_pair_classes_bf16: every row's destination pixel must lie inside the destination image");
  }
  RART_CHECK_ARG(!has2 || c->cls[0].src2, "rart_gemm_pair_classes_bf16: a second source needs class 0 to take it (src2 = 1)");
  return gp_launch(&h, has2 ? &c->two : nullptr, stream, c, plan_out, cus);
}
extern "C" int rart_gemm_pair_classes_bf16(const rart_gemm_pair_cls_desc* c, rart_stream_t stream) { return gp_launch_classes(c, stream, nullptr, 0); }

// The plan of the launching entry the descriptor belongs to (include/robustart_hip.h): that entry's checks, then steps 1 and 2 of gp_launch.
extern "C" int rart_gemm_pair_plan_bf16(const rart_gemm_pair_cls_desc* c, int cus, rart_gemm_pair_plan* out) {
  RART_CHECK_ARG(c != nullptr && out != nullptr, "rart_gemm_pair_plan_bf16: null descriptor or plan");
  return c->n_classes != 0 ? gp_launch_classes(c, nullptr, out, cus) : gp_launch2(&c->two, nullptr, out, cus);
}
