// Grouped 3x3 convolution, channels in = channels out, group widths 4 .. 64, bf16 or split-bf16 (hi + lo pair) NHWC (gfx950) -- conv2 of
// a ResNeXt Bottleneck (robustart_amd/model/resnet_torch.py with groups > 1), forward at stride 1 / 2 and backward-to-input (stride 1:
// flipped taps, per-group transposed weights; stride 2: one launch per input-parity class, 1 / 2 / 2 / 4 taps, strided destination).
//
// The channels are cut into SLICES of S = 32 consecutive channels (64 when the groups are 64 wide).  A slice holds whole groups, and as
// cin == cout the input and the output slice of a group coincide: slice s of the output reads slice s of the input and nothing else.
// The host lays the weights of a slice out as a dense [S out][taps][S in] table with exact zeros off the block diagonal, so a slice is a
// small dense convolution with K = taps * S.  The padded arithmetic (8 x at group width 4) is paid on the matrix cores; the launch moves
// every activation byte once.
//
// A workgroup owns one TH x 16 tile of output pixels of one image and one slice.  It stages the source pixels the tile reads -- the
// ((TH - 1) * stride + 3) x (15 * stride + 3) halo, zeros outside the image -- once for all taps, chunk major ([16-byte chunk][halo
// position], conv3x3_halo.hip's layout: the 16 pixels of a tile row are one contiguous run per chunk), then every wave walks taps x S / 16
// MFMA steps over its 2 (x MI) tile rows with the weight fragments streamed from L1 / L2 in fragment order.  No barrier in the K loop.
// One kernel text for both storages: PAIR stages the lo planes beside the hi planes and issues the three products hi.hi + hi.lo + lo.hi
// per step (as rart_gemm_pair_bf16 forms them); the epilogue (bias in the accumulators, 1-bit mask, ReLU, 1-bit sign of the stored hi
// value) works on the fp32 values and splits at the store.
#include "rart_common.h"
#include "rart_bf16_helpers.h"

namespace {
using namespace rart_bf16;

struct GroupedDesc {
  const uint16_t *src_hi, *src_lo;      // NHWC [n][src_h][src_w][channels]; lo: PAIR only
  const uint16_t *w_hi, *w_lo;          // fragment-ordered slice tables (see rart_conv3x3_grouped_bf16 in the header)
  const float* bias;                    // fp32 [channels] or null
  const uint8_t* mask_bits;             // 1 bit per destination element or null
  uint8_t* sign_out;                    // 1 bit per destination element or null
  uint16_t *dst_hi, *dst_lo;            // NHWC [n][dst_h][dst_w][channels]
  int src_h, src_w, channels, grid_h, grid_w, tiles_y, tiles_x, n_slices, n_taps;
  int tap_dy[9], tap_dx[9];
  int dst_h, dst_w, dst_s, dst_oy, dst_ox, relu;
};

constexpr int G_TW = 16;                // tile columns: one 16-pixel run per tile row
constexpr int G_LDW = 32 + 4;           // epilogue staging row (floats)

template <int S, bool PAIR, int STRIDE>
struct GCfg {
  static constexpr bool BIG = S == 64 && PAIR;                         // 256 bytes per staged pixel: the smaller tile keeps LDS under 64 KB
  static constexpr int WAVES = STRIDE == 1 ? 4 : (BIG ? 1 : 2);
  static constexpr int MI = (STRIDE == 1 && !BIG) ? 2 : 1;             // 32-pixel M tiles (2 tile rows) per wave
  static constexpr int TH = 2 * MI * WAVES;
  static constexpr int HH = (TH - 1) * STRIDE + 3, HW = (G_TW - 1) * STRIDE + 3, NPOS = HH * HW;
  static constexpr int CP = S / 8;                                     // 16-byte chunks per pixel and plane
  static constexpr int NPL = CP * (PAIR ? 2 : 1);                      // chunk planes: hi chunks, then lo chunks
  static constexpr int PLANE = (NPOS * 16 + 255) / 256 * 256 + 16;     // 16 mod 256: the chunks of one pixel fall in different bank slots
  static constexpr int HALO_BYTES = NPL * PLANE;
  static constexpr int STAGE_BYTES = WAVES * 32 * G_LDW * 4;
  static constexpr int LDS_BYTES = HALO_BYTES > STAGE_BYTES ? HALO_BYTES : STAGE_BYTES;
  static constexpr int NT = S / 32;                                    // 32-channel N tiles
  static constexpr int KS = S / 16;                                    // MFMA steps per tap
  static_assert(LDS_BYTES <= 64 * 1024, "static LDS");
};

template <int S, bool PAIR, int STRIDE>
__global__ __launch_bounds__((GCfg<S, PAIR, STRIDE>::WAVES * 64)) void k_conv3x3_grouped(const GroupedDesc d) {
  using C = GCfg<S, PAIR, STRIDE>;
  constexpr int T = C::WAVES * 64;
  __shared__ __attribute__((aligned(16))) uint8_t lds[C::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // logical ids contiguous per XCD: the slices of one tile share 128-byte lines of the source, tiles of one image share halo rows
  uint32_t t = rart_xcd_block(blockIdx.x, gridDim.x);
  const int slice = (int)(t % (uint32_t)d.n_slices);
  t /= (uint32_t)d.n_slices;
  const int tx = (int)(t % (uint32_t)d.tiles_x);
  t /= (uint32_t)d.tiles_x;
  const int ty = (int)(t % (uint32_t)d.tiles_y), img = (int)(t / (uint32_t)d.tiles_y);
  const int oy0 = ty * C::TH, ox0 = tx * G_TW;
  const int sy0 = oy0 * STRIDE - 1, sx0 = ox0 * STRIDE - 1;      // source pixel of halo position (0, 0)
  const int c0 = slice * S;

  // ---- the halo tile: every pixel the tile's taps can read, zeros outside the image
  {
    const size_t img_base = (size_t)img * d.src_h * d.src_w;
#pragma unroll 4
    for (int idx = tid; idx < C::NPOS * C::NPL; idx += T) {
      const int pl = idx % C::NPL, hp = idx / C::NPL;
      const int hr = hp / C::HW, hx = hp - hr * C::HW;
      const int y = sy0 + hr, x = sx0 + hx;
      uint4 v = make_uint4(0, 0, 0, 0);
      if ((unsigned)y < (unsigned)d.src_h && (unsigned)x < (unsigned)d.src_w) {
        const uint16_t* p = (PAIR && pl >= C::CP) ? d.src_lo : d.src_hi;
        v = *reinterpret_cast<const uint4*>(p + (img_base + (size_t)y * d.src_w + x) * d.channels + c0 + (pl % C::CP) * 8);
      }
      *reinterpret_cast<uint4*>(lds + pl * C::PLANE + hp * 16) = v;
    }
  }
  // ---- per-lane geometry: M tile i of the wave = tile rows (wave * MI + i) * 2 + {0, 1}, lane & 31 = row half * 16 + column
  const uint32_t kq = (uint32_t)(lane >> 5);          // which 8-k half of a 16-k MFMA step this lane supplies
  uint32_t abase[C::MI];
#pragma unroll
  for (int i = 0; i < C::MI; ++i) {
    const int p = lane & 31, row = (wave * C::MI + i) * 2 + (p >> 4), col = p & 15;
    abase[i] = (uint32_t)(((row * STRIDE + 1) * C::HW + col * STRIDE + 1) * 16) + kq * (uint32_t)C::PLANE;
  }
  f32x16 acc[C::MI][C::NT];
#pragma unroll
  for (int j = 0; j < C::NT; ++j) {
    const float bv = d.bias ? d.bias[c0 + j * 32 + (lane & 31)] : 0.f;
#pragma unroll
    for (int i = 0; i < C::MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = bv;
  }
  __syncthreads();

  // fragment (step st, N tile j) of the slice = 64 lanes x 8 elements: lane l -> T[j * 32 + (l & 31)][st * 16 + (l >> 5) * 8 ..]
  const size_t w_off = (size_t)slice * S * S * d.n_taps + (size_t)lane * 8;
  const uint16_t* wh = d.w_hi + w_off;
  const uint16_t* wl = PAIR ? d.w_lo + w_off : nullptr;
  for (int tap = 0; tap < d.n_taps; ++tap) {
    const int toff = (d.tap_dy[tap] * C::HW + d.tap_dx[tap]) * 16;
#pragma unroll
    for (int kc = 0; kc < C::KS; ++kc) {
      const int st = tap * C::KS + kc;
      bf16x8 bh[C::NT], bl[C::NT];
#pragma unroll
      for (int j = 0; j < C::NT; ++j) {
        bh[j] = *reinterpret_cast<const bf16x8*>(wh + (size_t)(st * C::NT + j) * 512);
        if (PAIR) bl[j] = *reinterpret_cast<const bf16x8*>(wl + (size_t)(st * C::NT + j) * 512);
      }
#pragma unroll
      for (int i = 0; i < C::MI; ++i) {
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(lds + (int)abase[i] + toff + (2 * kc) * C::PLANE);
        bf16x8 al;
        if (PAIR) al = *reinterpret_cast<const bf16x8*>(lds + (int)abase[i] + toff + (C::CP + 2 * kc) * C::PLANE);
#pragma unroll
        for (int j = 0; j < C::NT; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[j], acc[i][j], 0, 0, 0);
          if (PAIR) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[j], acc[i][j], 0, 0, 0);
          }
        }
      }
    }
  }
  __syncthreads();        // every wave is done reading the halo tile: its memory becomes the epilogue staging

  // ---- epilogue: each wave transposes a 32-pixel x 32-channel block through its private LDS slice and stores 16-byte row segments
  float* sE = reinterpret_cast<float*>(lds) + wave * 32 * G_LDW;
  const int cw = lane & 3, rw0 = lane >> 2;
#pragma unroll
  for (int i = 0; i < C::MI; ++i)
#pragma unroll
    for (int j = 0; j < C::NT; ++j) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sE[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * G_LDW + (lane & 31)] = acc[i][j][r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int oy = oy0 + (wave * C::MI + i) * 2 + q, ox = ox0 + rw0;      // staged row q * 16 + rw0
        if (oy < d.grid_h && ox < d.grid_w) {
          const float* sp = sE + (q * 16 + rw0) * G_LDW + cw * 8;
          const float4 v0 = *reinterpret_cast<const float4*>(sp), v1 = *reinterpret_cast<const float4*>(sp + 4);
          float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
          const size_t e = (((size_t)img * d.dst_h + (oy * d.dst_s + d.dst_oy)) * d.dst_w + (ox * d.dst_s + d.dst_ox)) * d.channels +
                           c0 + j * 32 + cw * 8;
          if (d.mask_bits) {
            const uint32_t mb = d.mask_bits[e >> 3];
#pragma unroll
            for (int k = 0; k < 8; ++k)
              if (!((mb >> k) & 1u)) v[k] = 0.f;
          }
          if (d.relu) {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
          }
          uint4 hi, lo;
          split8(v, hi, lo);
          *reinterpret_cast<uint4*>(d.dst_hi + e) = hi;
          if (PAIR) *reinterpret_cast<uint4*>(d.dst_lo + e) = lo;
          if (d.sign_out) d.sign_out[e >> 3] = (uint8_t)sign_byte(hi);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
}

int slice_width(int group_width) { return group_width == 64 ? 64 : 32; }

template <int S, bool PAIR, int STRIDE>
void launch_one(const GroupedDesc& d, int n, hipStream_t stream) {
  using C = GCfg<S, PAIR, STRIDE>;
  const dim3 grid((uint32_t)((long long)n * d.tiles_y * d.tiles_x * d.n_slices));
  hipLaunchKernelGGL((k_conv3x3_grouped<S, PAIR, STRIDE>), grid, dim3(C::WAVES * 64), 0, stream, d);
}

template <bool PAIR>
int tile_rows(int s, int stride) {
  if (s == 32) return stride == 1 ? GCfg<32, PAIR, 1>::TH : GCfg<32, PAIR, 2>::TH;
  return stride == 1 ? GCfg<64, PAIR, 1>::TH : GCfg<64, PAIR, 2>::TH;
}

template <bool PAIR>
int launch(const char* what, const void* src_hi, const void* src_lo, const void* w_hi, const void* w_lo, const float* bias,
           const void* mask_bits, void* sign_out, void* dst_hi, void* dst_lo, int n, int src_h, int src_w, int channels, int group_width,
           int stride, int grid_h, int grid_w, int n_taps, const int* tap_dy, const int* tap_dx, int dst_h, int dst_w, int dst_stride,
           int dst_oy, int dst_ox, int relu, rart_stream_t stream) {
  RART_CHECK_ARG(src_hi && w_hi && dst_hi && tap_dy && tap_dx && (!PAIR || (src_lo && w_lo && dst_lo)) && n > 0, "%s: bad arguments", what);
  RART_CHECK_ARG(src_hi != dst_hi && (!PAIR || (src_lo != dst_lo && src_hi != dst_lo && src_lo != dst_hi)),
                 "%s: dst must not alias src (workgroups read each other's halo pixels)", what);
  RART_CHECK_ARG(rart_conv3x3_grouped_supported(channels, group_width, src_h, src_w, stride),
                 "%s: unsupported geometry (group width 4 / 8 / 16 / 32 / 64 dividing the channels, channels a multiple of the slice, stride 1 or 2)", what);
  RART_CHECK_ARG(n_taps >= 1 && n_taps <= 9 && grid_h >= 1 && grid_w >= 1, "%s: 1 .. 9 taps, a non-empty grid", what);
  RART_CHECK_ARG(dst_stride >= 1 && dst_oy >= 0 && dst_ox >= 0 && (long long)(grid_h - 1) * dst_stride + dst_oy < dst_h &&
                 (long long)(grid_w - 1) * dst_stride + dst_ox < dst_w, "%s: the grid must map inside the destination", what);
  RART_CHECK_ARG((long long)n * src_h * src_w * channels < (1ll << 31) && (long long)n * dst_h * dst_w * channels < (1ll << 31),
                 "%s: tensors must stay below 2^31 elements", what);
  GroupedDesc d;
  d.src_hi = (const uint16_t*)src_hi; d.src_lo = (const uint16_t*)src_lo; d.w_hi = (const uint16_t*)w_hi; d.w_lo = (const uint16_t*)w_lo;
  d.bias = bias; d.mask_bits = (const uint8_t*)mask_bits; d.sign_out = (uint8_t*)sign_out;
  d.dst_hi = (uint16_t*)dst_hi; d.dst_lo = (uint16_t*)dst_lo;
  d.src_h = src_h; d.src_w = src_w; d.channels = channels; d.grid_h = grid_h; d.grid_w = grid_w; d.n_taps = n_taps;
  for (int t = 0; t < 9; ++t) d.tap_dy[t] = d.tap_dx[t] = 0;
  for (int t = 0; t < n_taps; ++t) {
    RART_CHECK_ARG(tap_dy[t] >= -1 && tap_dy[t] <= 1 && tap_dx[t] >= -1 && tap_dx[t] <= 1, "%s: taps must lie in -1..1", what);
    d.tap_dy[t] = tap_dy[t]; d.tap_dx[t] = tap_dx[t];
  }
  d.dst_h = dst_h; d.dst_w = dst_w; d.dst_s = dst_stride; d.dst_oy = dst_oy; d.dst_ox = dst_ox; d.relu = relu;
  const int s = slice_width(group_width), th = tile_rows<PAIR>(s, stride);
  d.n_slices = channels / s;
  d.tiles_y = (grid_h + th - 1) / th;
  d.tiles_x = (grid_w + G_TW - 1) / G_TW;
  RART_CHECK_ARG((long long)n * d.tiles_y * d.tiles_x * d.n_slices < (1ll << 31), "%s: too many tiles", what);
  const hipStream_t st = (hipStream_t)stream;
  if (s == 32 && stride == 1) launch_one<32, PAIR, 1>(d, n, st);
  else if (s == 32) launch_one<32, PAIR, 2>(d, n, st);
  else if (stride == 1) launch_one<64, PAIR, 1>(d, n, st);
  else launch_one<64, PAIR, 2>(d, n, st);
  RART_CHECK_LAUNCH(what);
  return RART_OK;
}
}  // namespace

extern "C" int rart_conv3x3_grouped_supported(int channels, int group_width, int h, int w, int stride) {
  if (group_width != 4 && group_width != 8 && group_width != 16 && group_width != 32 && group_width != 64) return 0;
  if (channels < 1 || channels % slice_width(group_width) != 0 || h < 1 || w < 1) return 0;
  return (stride == 1 || stride == 2) ? 1 : 0;
}

extern "C" int rart_conv3x3_grouped_tile(int group_width, int pair, int stride, int* rows, int* cols) {
  RART_CHECK_ARG(rows && cols && rart_conv3x3_grouped_supported(slice_width(group_width), group_width, 1, 1, stride),
                 "rart_conv3x3_grouped_tile: bad arguments");
  *rows = pair ? tile_rows<true>(slice_width(group_width), stride) : tile_rows<false>(slice_width(group_width), stride);
  *cols = G_TW;
  return RART_OK;
}

extern "C" int rart_conv3x3_grouped_bf16(const void* src, const void* wgt, const float* bias, const void* mask_bits, void* sign_out,
                                         void* dst, int n, int src_h, int src_w, int channels, int group_width, int stride, int grid_h,
                                         int grid_w, int n_taps, const int* tap_dy, const int* tap_dx, int dst_h, int dst_w,
                                         int dst_stride, int dst_oy, int dst_ox, int relu, rart_stream_t stream) {
  return launch<false>("rart_conv3x3_grouped_bf16", src, nullptr, wgt, nullptr, bias, mask_bits, sign_out, dst, nullptr, n, src_h, src_w,
                       channels, group_width, stride, grid_h, grid_w, n_taps, tap_dy, tap_dx, dst_h, dst_w, dst_stride, dst_oy, dst_ox,
                       relu, stream);
}

extern "C" int rart_conv3x3_grouped_pair(const void* src_hi, const void* src_lo, const void* wgt_hi, const void* wgt_lo, const float* bias,
                                         const void* mask_bits, void* sign_out, void* dst_hi, void* dst_lo, int n, int src_h, int src_w,
                                         int channels, int group_width, int stride, int grid_h, int grid_w, int n_taps,
                                         const int* tap_dy, const int* tap_dx, int dst_h, int dst_w, int dst_stride, int dst_oy,
                                         int dst_ox, int relu, rart_stream_t stream) {
  return launch<true>("rart_conv3x3_grouped_pair", src_hi, src_lo, wgt_hi, wgt_lo, bias, mask_bits, sign_out, dst_hi, dst_lo, n, src_h,
                      src_w, channels, group_width, stride, grid_h, grid_w, n_taps, tap_dy, tap_dx, dst_h, dst_w, dst_stride, dst_oy,
                      dst_ox, relu, stream);
}
