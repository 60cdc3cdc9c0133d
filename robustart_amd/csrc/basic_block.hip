// An identity BasicBlock (ResNet-18 / -34: two 3x3 stride-1 "same" convolutions C -> C and the identity skip) as ONE launch (gfx950),
// forward and backward-to-input:
//
//   forward :  out = relu(W2 * relu(W1 * x + b1) + b2 + x)       + sign bits of the intermediate and of out (each nullable)
//   backward:  dx  = m_in . (W1^T * (m_mid . (W2^T * g)) + g)     g = the masked gradient at the block output; m_in nullable
//
// Both directions are: 3x3, point-wise step, 3x3, + the kernel's own input, point-wise step -- one kernel text, the backward with the
// flipped taps and the transposed tables (the caller passes W2^T's table first).  Conv by conv the block moves five tensor passes
// through HBM (x, the intermediate out and in, x again as the residual, out); here the intermediate lives in LDS only and the residual
// comes from the staged x tile: two passes.
//
// A workgroup (8 waves) owns R = 7 output rows x TW columns of ONE image (TW = 56 at C = 64, 28 at C = 128: layer1 / layer2 at full
// width; wider images are cut into column tiles).  It stages the (R + 4) x (TW + 4) halo of x once -- rows and columns outside the image
// are zero, and a tile never reaches into a neighbouring image -- in the chunk-major planes of conv3x3_halo.hip (plane c = 16-byte
// chunk c of every position, plane stride 16 mod 256: the fragment read of 32 consecutive positions is one contiguous run and the chunk
// an immediate offset).  Stage 1 computes the intermediate on the R + 2 rows the second convolution reads, rounds it to bf16 ONCE
// (round-to-nearest-even, as a conv-by-conv chain would store it) and writes it into a second LDS tile of (R + 2) x (TW + 2) positions;
// stage 2 runs the second 3x3 from that tile.  INTERMEDIATE POSITIONS OUTSIDE THE IMAGE ARE ZERO -- they are the second convolution's
// zero padding, not relu(W1 * padded x + b1): the tile is zero-filled first, stage 1 computes image columns only and stores zero for
// rows outside the image.  Recompute factor (R + 2) / R = 1.29.
//
// The weight fragments (rart_conv3x3_pack_frag_bf16's order) stream from L1 / L2 one 64-deep K step ahead, as in conv3x3_halo.hip and
// conv_grouped.hip; there is no barrier inside a tap loop: one after staging, one between the stages.  The MFMA runs TRANSPOSED
// (A = weights, B = positions): a lane then holds four consecutive channels of ONE position per 4 accumulator registers, the position it
// also reads -- so the epilogue needs no LDS staging: lanes l and l ^ 32 swap halves and each owns whole 16-byte chunks (8 channels: one
// mask / sign byte), written to the intermediate tile or to global memory.
#include "rart_common.h"
#include "rart_bf16_helpers.h"

struct RartBasicDesc {
  const uint16_t* x;
  const uint16_t* w1;       // fragment-major [C][9 C] table of the first convolution
  const uint16_t* w2;       // ... of the second
  const float* b1;          // fp32 [C] or null
  const float* b2;
  uint8_t* m_mid;           // forward: sign bits of the intermediate (written, nullable); backward: its mask (read)
  uint8_t* m_io;            // forward: sign bits of out (written, nullable); backward: mask of dx (read, nullable)
  uint16_t* out;
  int n, h, w;
  int tiles_y, tiles_x;
  int tap_dy[9], tap_dx[9];
  int backward;
};

namespace {
using namespace rart_bf16;

template <int C>
struct BasicCfg {
  static constexpr int R = 7;                             // output rows per workgroup
  static constexpr int TW = C == 64 ? 56 : 28;            // output columns per workgroup
  static constexpr int T = 512;                           // threads: 8 waves
  static constexpr int CP = C / 8;                        // 16-byte chunks per position
  static constexpr int XW = TW + 4, MW = TW + 2;          // row strides of the x tile and of the intermediate tile, in positions
  static constexpr int XPOS = (R + 4) * XW, MPOS = (R + 2) * MW;
  static constexpr int XPLANE = ((XPOS + 15) / 16 * 16 + 1) * 16;
  static constexpr int MPLANE = ((MPOS + 15) / 16 * 16 + 1) * 16;
  static_assert(XPLANE % 256 == 16 && MPLANE % 256 == 16, "plane strides must be 16 mod 256");
  static constexpr int X_BYTES = CP * XPLANE, M_BYTES = CP * MPLANE;
  static constexpr int LDS_BYTES = X_BYTES + M_BYTES;
  static_assert(LDS_BYTES <= 160 * 1024, "both tiles must fit one workgroup's LDS");
  static constexpr int WAVES_N = C / 32;                  // waves along the channels (32 each): 2 / 4
  static constexpr int WAVES_M = 8 / WAVES_N;             // waves along the positions (groups of 128): 4 / 2
  static constexpr int KSTEPS = C / 64;
  static constexpr int STEPS = 9 * KSTEPS;
  static constexpr int WST = WAVES_N * 2048;              // table elements per 64-deep K step
};

// relu that keeps a NaN (v <= 0 is false for it): a poisoned input stays visible in every output that reads it
__device__ __forceinline__ float relu_keep_nan(float v) { return v <= 0.f ? 0.f : v; }

// One 3x3 over a group of 4 x 32 positions x the wave's 32 output channels, from the LDS tile `tile` (chunk-major planes of PLANE
// bytes, row stride `ws` positions): acc[i][4 j + t] += channel wn * 32 + 8 j + 4 (lane >> 5) + t of position i * 32 + (lane & 31).
// abase[i] = byte offset of that position's chunk (lane >> 5) in the tile.  wq: the wave's slice of the fragment table; loff = lane * 16,
// the lane's bytes within a fragment.  The table pointer WALKS from step to step behind an empty asm: with constant step offsets the
// compiler forms one 64-bit vector address per step ahead of the group loop -- 70 VGPRs at C = 128, which spilled.
template <int C, int PLANE>
__device__ __forceinline__ void conv_group(const uint8_t* tile, const uint32_t (&abase)[4], const uint16_t* wq, uint32_t loff, int ws,
                                           const RartBasicDesc& d, f32x16 (&acc)[4]) {
  using Cf = BasicCfg<C>;
  bf16x8 bq[2][4];
  const uint8_t* wp = reinterpret_cast<const uint8_t*>(wq) + loff;
  asm volatile("" : "+v"(wp));
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) bq[0][ks] = *reinterpret_cast<const bf16x8*>(wp + ks * 1024);
#pragma unroll
  for (int st = 0; st < Cf::STEPS; ++st) {
    const int tap = st / Cf::KSTEPS, kh = st % Cf::KSTEPS;
    if (st + 1 < Cf::STEPS) {
      wp += Cf::WST * 2;
      asm volatile("" : "+v"(wp));
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) bq[(st + 1) & 1][ks] = *reinterpret_cast<const bf16x8*>(wp + ks * 1024);
    }
    __builtin_amdgcn_sched_barrier(0);                    // keep the prefetch ahead of this step's MFMAs (see k_conv3x3_halo)
    const int toff = (d.tap_dy[tap] * ws + d.tap_dx[tap]) * 16;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 af[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[i] = *reinterpret_cast<const bf16x8*>(tile + (int)abase[i] + toff + (kh * 8 + ks * 2) * PLANE);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq[st & 1][ks], af[i], acc[i], 0, 0, 0);
    }
  }
}

__device__ __forceinline__ void init_acc(f32x16 (&acc)[4], const float* bias, int ch0) {
  float bv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) bv[r] = bias ? bias[ch0 + (r & 3) + 8 * (r >> 2)] : 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = bv[r];
}

// four packed channel quads d[j] (channels 8 j + 4 hi ..) of a lane's position -> the two whole 16-byte chunks the lane owns after the
// half swap with lane ^ 32: chunk 2 hi + jj, jj = 0, 1
__device__ __forceinline__ void swap_halves(const uint32_t (&dq)[4][2], int hi, uint32_t (&o)[2][4]) {
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    uint32_t own[2], recv[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      own[t] = hi ? dq[2 + jj][t] : dq[jj][t];
      const uint32_t send = hi ? dq[jj][t] : dq[2 + jj][t];
      recv[t] = (uint32_t)__shfl_xor((int)send, 32, 64);
    }
    o[jj][0] = hi ? recv[0] : own[0];
    o[jj][1] = hi ? recv[1] : own[1];
    o[jj][2] = hi ? own[0] : recv[0];
    o[jj][3] = hi ? own[1] : recv[1];
  }
}

template <int C>
__global__ __launch_bounds__(512, 1) void k_basic_block(const RartBasicDesc d) {
  using Cf = BasicCfg<C>;
  __shared__ __attribute__((aligned(16))) uint8_t lds[Cf::LDS_BYTES];
  uint8_t* const xt = lds;
  uint8_t* const mt = lds + Cf::X_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / Cf::WAVES_N, wn = wave % Cf::WAVES_N;
  const int hi = lane >> 5;
  const int H = d.h, W = d.w;
  // neighbouring tiles share halo rows: keep them on one XCD
  const uint32_t blk = rart_xcd_block(blockIdx.x, gridDim.x);
  const int per_img = d.tiles_y * d.tiles_x;
  const int img = (int)blk / per_img, trem = (int)blk - img * per_img;
  const int ty = trem / d.tiles_x, tx = trem - ty * d.tiles_x;
  const int r0 = ty * Cf::R, c0 = tx * Cf::TW;
  const int rv = min(Cf::R, H - r0), cv = min(Cf::TW, W - c0);       // output rows / columns this workgroup owns
  const uint32_t img_pos = (uint32_t)img * (uint32_t)H * (uint32_t)W;

  // ---- zero the intermediate tile, stage the x tile (every load of a thread in flight before its first LDS store)
  for (int idx = tid; idx < Cf::MPOS * Cf::CP; idx += Cf::T)
    *reinterpret_cast<uint4*>(mt + (idx & (Cf::CP - 1)) * Cf::MPLANE + (idx / Cf::CP) * 16) = make_uint4(0, 0, 0, 0);
  {
    constexpr int N_ITEMS = Cf::XPOS * Cf::CP;
    constexpr int U = (N_ITEMS + Cf::T - 1) / Cf::T;
    uint4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = u * Cf::T + tid;
      const int chunk = idx & (Cf::CP - 1), hp = idx / Cf::CP;
      const int hr = hp / Cf::XW, hx = hp - hr * Cf::XW;
      const int y = r0 - 2 + hr, x = c0 - 2 + hx;
      v[u] = make_uint4(0, 0, 0, 0);
      if (idx < N_ITEMS && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)
        v[u] = *reinterpret_cast<const uint4*>(d.x + ((size_t)img_pos + (size_t)y * W + x) * C + chunk * 8);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = u * Cf::T + tid;
      if (idx < N_ITEMS) *reinterpret_cast<uint4*>(xt + (idx & (Cf::CP - 1)) * Cf::XPLANE + (idx / Cf::CP) * 16) = v[u];
    }
  }
  __syncthreads();

  const int wn_s = __builtin_amdgcn_readfirstlane(wn);     // wave-uniform
  const uint32_t loff = (uint32_t)lane * 16u;
  const int ch0 = wn * 32 + 4 * hi;                        // the lane's first channel; its quads are ch0 + 8 j
  // ---- stage 1: the intermediate on rows r0 - 1 .. r0 + rv, image columns mc0 .. mc1 - 1 (the columns of the tile that exist)
  {
    const int mc0 = max(c0 - 1, 0), mc1 = min(c0 + cv + 1, W);
    const int mcols = mc1 - mc0, mshift = mc0 - (c0 - 1);
    const int P1 = (rv + 2) * mcols;
    const uint16_t* wq = d.w1 + wn_s * 2048;
    for (int g = wm; g * 128 < P1; g += Cf::WAVES_M) {
      uint32_t abase[4], mpos[4], epos[4];
      bool valid[4], inside[4], own[4];
      uint32_t mb[4][2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = g * 128 + i * 32 + (lane & 31);
        valid[i] = idx < P1;
        const int ic = valid[i] ? idx : P1 - 1;             // lanes past the end read a real position and store nothing
        const int row = ic / mcols, col = ic - row * mcols;
        const int y = r0 - 1 + row, x = mc0 + col;
        inside[i] = (unsigned)y < (unsigned)H;
        own[i] = row >= 1 && row <= rv && x >= c0 && x < c0 + cv;
        abase[i] = (uint32_t)(((row + 1) * Cf::XW + mshift + col + 1) * 16 + hi * Cf::XPLANE);
        mpos[i] = (uint32_t)((row * Cf::MW + mshift + col) * 16);
        epos[i] = inside[i] ? img_pos + (uint32_t)(y * W + x) : 0u;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
          mb[i][jj] = (d.backward && valid[i] && inside[i]) ? d.m_mid[(size_t)epos[i] * Cf::CP + wn * 4 + hi * 2 + jj] : 0xFFu;
      }
      f32x16 acc[4];
      init_acc(acc, d.b1, ch0);
      conv_group<C, Cf::XPLANE>(xt, abase, wq, loff, Cf::XW, d, acc);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t dq[4][2], o[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = d.backward ? acc[i][4 * j + t] : relu_keep_nan(acc[i][4 * j + t]);
          dq[j][0] = pack_bf16x2(v[0], v[1]);
          dq[j][1] = pack_bf16x2(v[2], v[3]);
        }
        swap_halves(dq, hi, o);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const int q = wn * 4 + hi * 2 + jj;
          if (d.backward) {
#pragma unroll
            for (int t = 0; t < 4; ++t) o[jj][t] &= halves_from_bits(mb[i][jj], t);
          }
          const uint4 ov = inside[i] ? make_uint4(o[jj][0], o[jj][1], o[jj][2], o[jj][3]) : make_uint4(0, 0, 0, 0);
          if (valid[i]) *reinterpret_cast<uint4*>(mt + q * Cf::MPLANE + mpos[i]) = ov;
          if (!d.backward && d.m_mid && valid[i] && own[i]) d.m_mid[(size_t)epos[i] * Cf::CP + q] = (uint8_t)sign_byte(ov);
        }
      }
    }
  }
  __syncthreads();

  // ---- stage 2: the second 3x3 from the intermediate tile, + bias + the staged x, point-wise step, store
  {
    const int P2 = rv * cv;
    const uint16_t* wq = d.w2 + wn_s * 2048;
    for (int g = wm; g * 128 < P2; g += Cf::WAVES_M) {
      uint32_t abase[4], xpos[4], epos[4];
      bool valid[4];
      uint32_t mb[4][2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = g * 128 + i * 32 + (lane & 31);
        valid[i] = idx < P2;
        const int ic = valid[i] ? idx : P2 - 1;
        const int row = ic / cv, col = ic - row * cv;
        abase[i] = (uint32_t)(((row + 1) * Cf::MW + col + 1) * 16 + hi * Cf::MPLANE);
        xpos[i] = (uint32_t)(((row + 2) * Cf::XW + col + 2) * 16 + hi * 8);
        epos[i] = img_pos + (uint32_t)((r0 + row) * W + c0 + col);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
          mb[i][jj] = (d.backward && d.m_io && valid[i]) ? d.m_io[(size_t)epos[i] * Cf::CP + wn * 4 + hi * 2 + jj] : 0xFFu;
      }
      f32x16 acc[4];
      init_acc(acc, d.b2, ch0);
      conv_group<C, Cf::MPLANE>(mt, abase, wq, loff, Cf::MW, d, acc);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t dq[4][2], o[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          // the residual: the lane's four channels of its own position, from the x tile
          const uint2 xr = *reinterpret_cast<const uint2*>(xt + (wn * 4 + j) * Cf::XPLANE + xpos[i]);
          float v[4];
          v[0] = acc[i][4 * j + 0] + __uint_as_float(xr.x << 16);
          v[1] = acc[i][4 * j + 1] + __uint_as_float(xr.x & 0xFFFF0000u);
          v[2] = acc[i][4 * j + 2] + __uint_as_float(xr.y << 16);
          v[3] = acc[i][4 * j + 3] + __uint_as_float(xr.y & 0xFFFF0000u);
          if (!d.backward) {
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = relu_keep_nan(v[t]);
          }
          dq[j][0] = pack_bf16x2(v[0], v[1]);
          dq[j][1] = pack_bf16x2(v[2], v[3]);
        }
        swap_halves(dq, hi, o);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const int q = wn * 4 + hi * 2 + jj;
          if (d.backward) {
#pragma unroll
            for (int t = 0; t < 4; ++t) o[jj][t] &= halves_from_bits(mb[i][jj], t);
          }
          const uint4 ov = make_uint4(o[jj][0], o[jj][1], o[jj][2], o[jj][3]);
          if (valid[i]) {
            *reinterpret_cast<uint4*>(d.out + (size_t)epos[i] * C + q * 8) = ov;
            if (!d.backward && d.m_io) d.m_io[(size_t)epos[i] * Cf::CP + q] = (uint8_t)sign_byte(ov);
          }
        }
      }
    }
  }
}
}  // namespace

// 1 if rart_basic_block_bf16 runs an identity BasicBlock of this width on h x w images
extern "C" int rart_basic_block_supported(int channels, int h, int w) {
  return ((channels == 64 || channels == 128) && h >= 1 && w >= 1) ? 1 : 0;
}

// the output pixels one workgroup owns (rows x cols of one image); RART_ERR_INVALID for a width the kernel does not take
extern "C" int rart_basic_block_tile(int channels, int* rows, int* cols) {
  RART_CHECK_ARG(rows && cols, "rart_basic_block_tile: null pointer");
  RART_CHECK_ARG(channels == 64 || channels == 128, "rart_basic_block_tile: channels must be 64 or 128");
  *rows = channels == 64 ? BasicCfg<64>::R : BasicCfg<128>::R;
  *cols = channels == 64 ? BasicCfg<64>::TW : BasicCfg<128>::TW;
  return RART_OK;
}

extern "C" int rart_basic_block_bf16(const void* x, const void* w1, const void* w2, const float* b1, const float* b2, void* m_mid,
                                     void* m_io, void* out, int n, int h, int w, int channels, const int* tap_dy, const int* tap_dx,
                                     int backward, rart_stream_t stream) {
  RART_CHECK_ARG(x && w1 && w2 && out && tap_dy && tap_dx, "rart_basic_block_bf16: null tensor");
  RART_CHECK_ARG(backward == 0 || backward == 1, "rart_basic_block_bf16: backward must be 0 or 1");
  RART_CHECK_ARG(!backward || m_mid, "rart_basic_block_bf16: null tensor (the backward reads the intermediate's mask)");
  RART_CHECK_ARG(n > 0, "rart_basic_block_bf16: n must be positive");
  RART_CHECK_ARG(rart_basic_block_supported(channels, h, w), "rart_basic_block_bf16: unsupported geometry (channels 64 / 128, h and w >= 1)");
  RART_CHECK_ARG((long long)n * h * w * channels < (1ll << 31), "rart_basic_block_bf16: tensor must stay below 2^31 elements");
  RART_CHECK_ARG(x != out, "rart_basic_block_bf16: out must not alias x (workgroups read each other's halo rows)");
  RART_CHECK_ARG(((uintptr_t)x | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)out) % 16 == 0 && ((uintptr_t)b1 | (uintptr_t)b2) % 4 == 0,
                 "rart_basic_block_bf16: tensors must be 16-byte aligned, biases 4-byte aligned");
  RartBasicDesc d;
  d.x = (const uint16_t*)x; d.w1 = (const uint16_t*)w1; d.w2 = (const uint16_t*)w2; d.b1 = b1; d.b2 = b2;
  d.m_mid = (uint8_t*)m_mid; d.m_io = (uint8_t*)m_io; d.out = (uint16_t*)out;
  d.n = n; d.h = h; d.w = w; d.backward = backward;
  for (int t = 0; t < 9; ++t) {
    RART_CHECK_ARG(tap_dy[t] >= -1 && tap_dy[t] <= 1 && tap_dx[t] >= -1 && tap_dx[t] <= 1, "rart_basic_block_bf16: taps must lie in -1..1");
    d.tap_dy[t] = tap_dy[t]; d.tap_dx[t] = tap_dx[t];
  }
  const int R = channels == 64 ? BasicCfg<64>::R : BasicCfg<128>::R, TW = channels == 64 ? BasicCfg<64>::TW : BasicCfg<128>::TW;
  d.tiles_y = (h + R - 1) / R;
  d.tiles_x = (w + TW - 1) / TW;
  const long long blocks = (long long)n * d.tiles_y * d.tiles_x;
  RART_CHECK_ARG(blocks < (1ll << 31), "rart_basic_block_bf16: too many tiles");
  const dim3 grid((uint32_t)blocks);
  if (channels == 64) hipLaunchKernelGGL(k_basic_block<64>, grid, dim3(512), 0, (hipStream_t)stream, d);
  else hipLaunchKernelGGL(k_basic_block<128>, grid, dim3(512), 0, (hipStream_t)stream, d);
  RART_CHECK_LAUNCH("rart_basic_block_bf16");
  return RART_OK;
}
