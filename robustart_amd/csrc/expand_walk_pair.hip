// The short-K wide 1x1 pair products of ResNet-50's identity blocks (layer3: 50176 x 256 -> 1024 at B = 256; the expansion with its skip
// pair, ReLU and sign bytes, and conv1^T with the gradient pair as residual and a 1-bit mask) with the A rows RESIDENT IN REGISTERS.
//
// rart_gemm_pair_bf16 runs these launches on k_gemm_pair<256, 64, conv>: N / 64 = 16 column tiles per row tile, each its own workgroup
// that stages the row tile's A planes again -- 0.8 GB of A through the texture-address unit per launch for 51 MB of tensor.  Here a
// workgroup owns TR rows (TR / 32 waves, 32 rows each) and walks the columns in chunks of 64 -- all of them, or one of `parts` equal
// shares (finer units for the dispatcher; A then goes through the load path `parts` times):
//   * every wave loads the MFMA A fragments of its 32 rows for the whole K once, hi and lo plane: 8 VGPRs per 16-deep sub-step, 128 at
//     K = 256 (a lane's fragment of sub-step s is the 16 bytes at k = 16 s + 8 (lane >> 5) of row lane & 31: straight from global memory);
//   * per chunk and 32-deep K step the W stage (64 columns x 64 B x hi / lo = 8 KB) goes global -> LDS through rart_lds_dma.h's buffer
//     loads in k_gemm_pair's swizzled image (same fragment reads).  Registers allow two waves per SIMD, so nothing but distance hides a
//     stage's latency: FOUR stages in LDS, requested three K steps ahead, with counted waits;
//   * multiply order per accumulator as in k_gemm_pair: kt ascending, ks, then lo.hi, hi.lo, hi.hi into one fp32 accumulator that starts
//     at the bias -- and the 32 x 64 block of a chunk is finished by gp_finish_segment (rart_gemm_pair_dev.h): every output bit equals
//     rart_gemm_pair_bf16's;
//   * the stage requests run on across the chunk's end, the epilogue's operands are requested two K steps before it, and its
//     transposition has an LDS region of its own (TR / 32 x 8.5 KB), so it never waits for the workgroup.
// Measured at B = 256 (profiles/expand_walk_ab.json): 148 -> 135 us at layer3's shape, 217 -> 199 us at layer2's.
// Geometry: what these launches use -- conv mode, one tap at (0, 0), stride 1, source = row grid = destination, ldc = N: row m reads
// source pixel m and writes destination pixel m.
#include "rart_common.h"

#include "rart_gemm_pair_dev.h"
#include "rart_lds_dma.h"

namespace {
constexpr int EW_STAGE = 2 * 64 * GP_BK * 2;      // a W stage: 64 columns x 64 B, hi plane then lo plane (8 KB)
constexpr int EW_MAX_K = 256;
constexpr int EW_RING = 4;                        // W stages in LDS: stage t sits in buffer t % 4 and is requested three K steps ahead

template <int TR, int K>
__global__ __launch_bounds__(TR * 2, 2) void k_expand_walk_pair(const GemmPairDev d, const int parts) {
  constexpr int NW = TR / 32, KT = K / GP_BK, KS = K / 16;
  constexpr int WQ = 8 / NW;                        // 1 KiB pieces (16 columns x 64 B) of a W stage per wave: 2 (TR = 128) or 4 (TR = 64)
  __shared__ __attribute__((aligned(16))) uint8_t lds[EW_RING * EW_STAGE + NW * 32 * GP_LDE * 4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 31, h = lane >> 5;
  // The column chunks of a row tile go to `parts` workgroups (finer units for the dispatcher: 392 row tiles of layer3 at B = 256 on 512
  // resident workgroups leave every other CU with half the rows of its neighbour).  Row tiles are enumerated in groups of eight and
  // workgroup i goes to XCD i % 8: the parts of a row tile follow each other on one XCD, whose L2 serves the later ones' A rows.
  const int slot = blockIdx.x >> 3, m_tile = (slot / parts) * 8 + (blockIdx.x & 7), part = slot % parts;
  if (m_tile * TR >= d.M) return;
  const int m0 = m_tile * TR + wave * 32;           // the wave's first row
  const int c0 = part * (d.N / 64 / parts), c1 = c0 + d.N / 64 / parts;       // the workgroup's column chunks

  // ---- W loader: a plane of a stage goes to LDS in four 1 KiB pieces (16 columns x 64 B); wave w brings the pieces w, w + NW, .. of both
  //      planes; lane -> column (lane >> 2) of the piece, LDS chunk (lane & 3) <- the row's chunk (lane & 3) ^ ((column >> 2) & 3).  The
  //      chunk of columns and the K step move the scalar offset.
  static_assert(KT % EW_RING == 0, "stage c * KT + kt sits in buffer kt % EW_RING");
  uint32_t wvoff[WQ / 2];
#pragma unroll
  for (int q = 0; q < WQ / 2; ++q) {
    const int r = 16 * (wave + NW * q) + (lane >> 2);
    wvoff[q] = (uint32_t)((r * d.ldw + (((lane & 3) ^ ((r >> 2) & 3)) * 8)) * 2);
  }
  const rart_srd_t srd_wh = rart_dma_srd(d.w_hi), srd_wl = rart_dma_srd(d.w_lo);
  // (the resource words come from v_readfirstlane: the wait states between that write and the first buffer load that reads them)
  asm volatile("s_nop 4" : : "s"(srd_wh), "s"(srd_wl));
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)lds;
  const uint32_t chunk_bytes = (uint32_t)(64 * d.ldw * 2);
  auto issue = [&](int chunk, int kt, int buf) {
    const uint32_t so = (uint32_t)chunk * chunk_bytes + (uint32_t)kt * 64u;
#pragma unroll
    for (int q = 0; q < WQ / 2; ++q) {
      const uint32_t at = lds_base + buf * EW_STAGE + (wave + NW * q) * 1024;
      rart_dma_load16(wvoff[q], srd_wh, so, at);
      rart_dma_load16(wvoff[q], srd_wl, so, at + EW_STAGE / 2);
    }
  };
  issue(c0, 0, 0);
  issue(c0, 1, 1);
  issue(c0, 2, 2);

  // ---- A: the wave's fragments of the whole K, loaded once (rows past M read the last row: their results are never stored)
  bf16x8 ah[KS], al[KS];
  {
    const int m = min(m0 + fr, d.M - 1);
    const size_t at = (size_t)m * d.lda + 8 * h;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      ah[s] = *reinterpret_cast<const bf16x8*>(d.a_hi + at + 16 * s);
      al[s] = *reinterpret_cast<const bf16x8*>(d.a_lo + at + 16 * s);
    }
  }
  uint32_t xo[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) xo[ks] = (uint32_t)(fr * 64 + (((2 * ks + h) ^ ((fr >> 2) & 3)) << 4));

  // ---- epilogue geometry (gp_epilogue's: lane -> 8-column segment cw of row q * 8 + rw of the wave's 32 x 64 block)
  float* sE = reinterpret_cast<float*>(lds + EW_RING * EW_STAGE) + wave * 32 * GP_LDE;
  const int cw = lane & 7, rw = lane >> 3;
  const int flags = d.flags;
  long long erow[4], lrow[4];             // element offset of the segment's row: -1 past M (stores) / the last row's (loads)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int m = m0 + q * 8 + rw;
    erow[q] = m < d.M ? (long long)m * d.ldc : -1;
    lrow[q] = (long long)min(m, d.M - 1) * d.ldc;
  }

  // what a chunk's epilogue reads, in loads per lane (wave-uniform): the residual pair, the mask bytes, the next chunk's bias
  const int n_eload = (d.res_hi ? 8 : 0) + (d.mask_bits ? 4 : 0) + (d.bias ? 2 : 0);
  float bnext[2] = {0.f, 0.f};              // the bias of the next chunk's columns (lane & 31 is the column of a 32 x 32 MFMA tile)
  if (d.bias) {
    bnext[0] = d.bias[c0 * 64 + fr];
    bnext[1] = d.bias[c0 * 64 + 32 + fr];
  }
  rart_dma_wait<0>();
  __builtin_amdgcn_s_waitcnt(0x0F70);       // (the same wait as a builtin: the compiler then knows its own loads above have landed)
  __syncthreads();
  for (int c = c0; c < c1; ++c) {
    // accumulators start at the bias of their column
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = bnext[j];
    const int col = c * 64 + cw * 8;
    uint4 rh[4], rl[4];
    uint32_t mb[4];
    const bool more = c + 1 < c1;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const int buf = kt % EW_RING;
      if (kt == KT - 2) {
        // the epilogue's residual / mask operands are requested two K steps early (straight-line loads; rows past M read the last row)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const long long e = lrow[q] + col;
          rh[q] = rl[q] = make_uint4(0, 0, 0, 0);
          mb[q] = 0xFFu;
          if (d.res_hi) {
            rh[q] = gp_nt_load(d.res_hi + e);
            rl[q] = gp_nt_load(d.res_lo + e);
          }
          if (d.mask_bits) mb[q] = d.mask_bits[e >> 3];
        }
        if (d.bias) {            // (past the last chunk: the last chunk's again, unused)
          const int cn = min(c + 1, c1 - 1) * 64 + fr;
          bnext[0] = d.bias[cn];
          bnext[1] = d.bias[cn + 32];
        }
      }
      // stage t + 3 goes into the buffer that stage t - 1 left at the last barrier; past the chunk's end: the next chunk's first stages
      const bool issued = kt + 3 < KT || more;
      if (kt + 3 < KT) issue(c, kt + 3, (kt + 3) % EW_RING);
      else if (more) issue(c + 1, kt + 3 - KT, (kt + 3) % EW_RING);
      const uint8_t* Bh = lds + buf * EW_STAGE;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 bh[2], bl[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          bh[j] = *reinterpret_cast<const bf16x8*>(Bh + j * 32 * 64 + xo[ks]);
          bl[j] = *reinterpret_cast<const bf16x8*>(Bh + EW_STAGE / 2 + j * 32 * 64 + xo[ks]);
        }
        // the two small products first, the large one last: all three land in the same fp32 accumulator
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[2 * kt + ks], bh[j], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[2 * kt + ks], bl[j], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[2 * kt + ks], bh[j], acc[j], 0, 0, 0);
        }
      }
      // Stage t + 1 has landed once at most the LOADS requested after it are outstanding (loads complete in order; a pending store of
      // the last epilogue only makes the wait longer): the stages t + 2 and t + 3, and from step KT - 2 on the epilogue's operands.
      // Steps 0 and 1 wait for nothing: their next stages landed before the last epilogue's (the prologue's) full wait, which every
      // wave has passed at this barrier.
      if (kt >= 2) {
        if (!issued) rart_dma_wait<0>();
        else if (kt < KT - 2) rart_dma_wait<2 * WQ>();
        else switch (n_eload) {
          case 0: rart_dma_wait<2 * WQ>(); break;
          case 2: rart_dma_wait<2 * WQ + 2>(); break;
          case 4: rart_dma_wait<2 * WQ + 4>(); break;
          case 6: rart_dma_wait<2 * WQ + 6>(); break;
          case 8: rart_dma_wait<2 * WQ + 8>(); break;
          case 10: rart_dma_wait<2 * WQ + 10>(); break;
          case 12: rart_dma_wait<2 * WQ + 12>(); break;
          default: rart_dma_wait<2 * WQ + 14>(); break;
        }
      }
      __syncthreads();
    }
    // ---- the chunk's 32 x 64 block of this wave through its own LDS region
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) sE[((r & 3) + 8 * (r >> 2) + 4 * h) * GP_LDE + j * 32 + fr] = acc[j][r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // vmcnt(0) as a builtin the compiler counts (the epilogue's operands, and the stages requested so far): with stores pending it
    // otherwise waits for ALL of a segment's stores before it reads the next segment's operands (loads and stores share the counter)
    __builtin_amdgcn_s_waitcnt(0x0F70);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = q * 8 + rw;
      const float4 v0 = *reinterpret_cast<const float4*>(sE + r * GP_LDE + cw * 8);
      const float4 v1 = *reinterpret_cast<const float4*>(sE + r * GP_LDE + cw * 8 + 4);
      if (erow[q] >= 0) {
        float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        const uint4 none = make_uint4(0, 0, 0, 0);
        gp_finish_segment<true, false>(d, flags, false, erow[q] + col, v, rh[q], rl[q], none, none, mb[q]);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// what tile_rows = 0 / col_parts = 0 stand for, from the kernel-alone A/B at B = 256 (profiles/expand_walk_ab.json): 128-row tiles; the
// columns of a row tile in four workgroups at K = 256 (layer3: 392 row tiles), in two at K = 128 (layer2: 1568)
constexpr int EW_DEFAULT_ROWS = 128;
int ew_default_parts(int K) { return K > 128 ? 4 : 2; }
}  // namespace

extern "C" int rart_expand_walk_pair_max_k(void) { return EW_MAX_K; }

extern "C" int rart_expand_walk_pair(const rart_gemm_pair_desc* h, int tile_rows, int col_parts, rart_stream_t stream) {
  RART_CHECK_ARG(h != nullptr, "rart_expand_walk_pair: null descriptor");
  RART_CHECK_ARG(h->a_hi && h->a_lo && h->w_hi && h->w_lo && h->dst_hi && h->dst_lo, "rart_expand_walk_pair: null operand plane (the destination is a pair)");
  RART_CHECK_ARG(tile_rows == 0 || tile_rows == 64 || tile_rows == 128, "rart_expand_walk_pair: tile_rows must be 0 (default), 64 or 128");
  RART_CHECK_ARG(col_parts == 0 || col_parts == 1 || col_parts == 2 || col_parts == 4, "rart_expand_walk_pair: col_parts must be 0 (default), 1, 2 or 4");
  RART_CHECK_ARG(h->conv != 0 && h->n_taps == 1 && h->tap_dy[0] == 0 && h->tap_dx[0] == 0 && h->sy == 1 && h->sx == 1,
                 "rart_expand_walk_pair: conv mode, one tap at (0, 0), stride 1");
  RART_CHECK_ARG(h->batch > 0 && h->grid_h > 0 && h->grid_w > 0 && h->src_h == h->grid_h && h->src_w == h->grid_w && h->dst_h == h->grid_h &&
                     h->dst_w == h->grid_w && h->dst_sy == 1 && h->dst_sx == 1 && h->dst_oy == 0 && h->dst_ox == 0,
                 "rart_expand_walk_pair: source, row grid and destination must be the same pixels");
  RART_CHECK_ARG(h->n_batched <= 1 && h->rows_per_image == 0 && h->src_row_off == 0 && h->dst_row_off == 0,
                 "rart_expand_walk_pair: no batching / row re-basing");
  const int K = h->k_per_tap;
  RART_CHECK_ARG(K == 128 || K == 256, "rart_expand_walk_pair: K must be 128 or 256 (rart_expand_walk_pair_max_k; the A rows live in registers)");
  RART_CHECK_ARG(h->N >= 64 && h->N % 64 == 0 && h->ldc == h->N, "rart_expand_walk_pair: N must be a positive multiple of 64 and ldc = N");
  RART_CHECK_ARG(h->w_rows == 0 || h->w_rows >= h->N, "rart_expand_walk_pair: the weight table must hold N rows");
  RART_CHECK_ARG(h->lda % 8 == 0 && h->lda >= K && h->ldw % 8 == 0 && h->ldw >= K, "rart_expand_walk_pair: lda / ldw must cover K and keep 16-byte alignment");
  const long long M = (long long)h->batch * h->grid_h * h->grid_w;
  RART_CHECK_ARG(M * h->lda < (1ll << 30) && M * h->N < (1ll << 31) && (long long)h->N * h->ldw < (1ll << 30),
                 "rart_expand_walk_pair: a source or weight plane must stay below 2 GiB and the destination below 2^31 elements (split the batch)");
  RART_CHECK_ARG((h->res_hi == nullptr) == (h->res_lo == nullptr), "rart_expand_walk_pair: the residual is a pair: both planes or none");
  RART_CHECK_ARG(!(h->flags & ~GP_RELU) && !h->aux_hi && !h->aux_lo, "rart_expand_walk_pair: flags other than ReLU and the GELU operands are not served");
  GemmPairDev d{};
  d.a_hi = (const uint16_t*)h->a_hi; d.a_lo = (const uint16_t*)h->a_lo; d.w_hi = (const uint16_t*)h->w_hi; d.w_lo = (const uint16_t*)h->w_lo;
  d.bias = h->bias; d.res_hi = (const uint16_t*)h->res_hi; d.res_lo = (const uint16_t*)h->res_lo;
  d.dst_hi = (uint16_t*)h->dst_hi; d.dst_lo = (uint16_t*)h->dst_lo;
  d.M = (int)M; d.N = h->N; d.K = K; d.lda = h->lda; d.ldw = h->ldw; d.ldc = h->ldc; d.w_rows = h->N;
  d.flags = h->flags;
  d.mask_bits = (const uint8_t*)h->mask_bits; d.sign_out = (uint8_t*)h->sign_out;
  d.nt = 1;                                   // the residual and output streams of these launches never fit an XCD's L2
  const int tr = tile_rows ? tile_rows : EW_DEFAULT_ROWS;
  int parts = col_parts ? col_parts : ew_default_parts(K);
  RART_CHECK_ARG(col_parts == 0 || (h->N / 64) % col_parts == 0, "rart_expand_walk_pair: col_parts must divide the N / 64 column chunks");
  while ((h->N / 64) % parts) parts /= 2;
  const long long m_tiles = (M + tr - 1) / tr;
  const dim3 grid((unsigned)((m_tiles + 7) / 8 * 8 * parts));
  hipStream_t st = (hipStream_t)stream;
  if (tr == 128) {
    if (K == 256) hipLaunchKernelGGL((k_expand_walk_pair<128, 256>), grid, dim3(256), 0, st, d, parts);
    else hipLaunchKernelGGL((k_expand_walk_pair<128, 128>), grid, dim3(256), 0, st, d, parts);
  } else {
    if (K == 256) hipLaunchKernelGGL((k_expand_walk_pair<64, 256>), grid, dim3(128), 0, st, d, parts);
    else hipLaunchKernelGGL((k_expand_walk_pair<64, 128>), grid, dim3(128), 0, st, d, parts);
  }
  RART_CHECK_LAUNCH("rart_expand_walk_pair");
  return RART_OK;
}
