// Training-side kernels of the ConvNeXt-B train engine (robustart_amd/model/convnext_train_engine.py) for gfx950: the 7x7 depthwise
// convolution's weight and bias gradient and the layer scale (`gamma`) forward / backward.  bf16 storage, fp32 arithmetic; activations
// NHWC [n][h][w][c] = [rows][c], the layout of every other ConvNeXt kernel (csrc/convnext.hip).
//
// Depthwise weight gradient, dw[dy * 7 + dx][c] = sum over (image, y, x) of x[y + dy - 3][x + dx - 3][c] * dz[y][x][c], db[c] = sum dz:
//   * Unlike the fused forward, nothing here needs every channel of a pixel in one workgroup, so a workgroup owns a 32-channel slice
//     of a strip of output rows of one or more images and keeps a rolling window of the 7 input rows those output rows read in LDS
//     ([7][w + 6][32] bf16, the three zero columns of padding on each side written once) plus the current dz row ([w][32]).  Moving to
//     the next output row loads ONE new input row: inside a strip every input element is fetched once, and the strip's 6 halo rows
//     are the only re-reads (strips of <= 14 rows; the neighbouring strip's copy is usually still in L2).  The next row's two new
//     rows are fetched into registers while the current row is computed.
//   * Thread (channel, dy) -- 32 x 7 of the 256 -- slides a 7-element register window along input row y + dy - 3 and accumulates the 7
//     taps dx of its row dy: one LDS read of x and one of dz per 7 FMAs.  The dy = 3 thread (its row is always inside the image) also
//     sums dz for the bias.
//   * Determinism: no atomics.  Each workgroup writes its 49 + 1 fp32 sums per channel to its own slot of a partial buffer and
//     k_fold adds the slots in a fixed order; the geometry (strip height, images per workgroup) depends on the shape alone, so the same
//     inputs give bit-identical outputs on every call.
// Layer scale: the block output is x_out = x_in + gamma * u2 with u2 = fc2(gelu(fc1(LN(dwconv(x_in))))) KEPT unscaled.  The backward
// forms dgamma = sum_rows dx * u2 and dv = gamma * dx (fc2's output gradient) -- gamma is never divided out and u2 is never recovered
// as x_out - x_in: at timm's initial gamma of 1e-6 both would lose every bit.  Reductions as above: per-workgroup partials, one fold.
// Reference: torch autograd through timm's ConvNeXt block (conv_dw, LayerNorm, fc1, GELU, fc2, gamma, residual), restated in
// robustart_amd/model/convnext_torch.py; the adversarial-training configs exprs/nips_benchmark/{pgd,new}_adv_train/convnext_base.
#include "rart_common.h"
#include "rart_bf16_helpers.h"

namespace {
using namespace rart_bf16;
constexpr int kBlock = 256;
constexpr int kSlice = 32;                      // channels per workgroup of the depthwise weight gradient
constexpr int kTaps = 49;
constexpr int kDwRows = kTaps + 1;              // partial rows per workgroup: 49 taps + the bias
constexpr int kStripRows = 14;                  // output rows per strip (at most)
constexpr int kMaxW = 128;                      // LDS window: (7 * (w + 6) + w) * 32 * 2 bytes = 68 KB at w = 128
constexpr int kTargetWgs = 1024;

struct DwGeom {
  int strip_rows, strips, imgs_per_wg, groups, slices;
};

DwGeom dw_geom(int n, int h, int c) {
  DwGeom g;
  g.strips = (h + kStripRows - 1) / kStripRows;
  g.strip_rows = (h + g.strips - 1) / g.strips;
  g.slices = (c + kSlice - 1) / kSlice;
  const long long base = (long long)n * g.strips * g.slices;
  g.imgs_per_wg = (int)(base / kTargetWgs > 1 ? base / kTargetWgs : 1);
  if (g.imgs_per_wg > n) g.imgs_per_wg = n;
  g.groups = (n + g.imgs_per_wg - 1) / g.imgs_per_wg;
  return g;
}

// one input row (y) of the channel slice -> LDS window slot, interior columns 3 .. w + 2 (8-byte pieces of 4 channels)
__device__ __forceinline__ void dw_load_row(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int W, int C, int c0) {
  for (int i = threadIdx.x; i < W * (kSlice / 4); i += kBlock) {
    const int col = i / (kSlice / 4), q = i % (kSlice / 4);
    uint2 v = make_uint2(0u, 0u);
    if (c0 + 4 * q < C) v = *reinterpret_cast<const uint2*>(src + (size_t)col * C + c0 + 4 * q);
    *reinterpret_cast<uint2*>(dst + col * kSlice + 4 * q) = v;
  }
}

constexpr int kPf = kMaxW * (kSlice / 4) / kBlock;    // 8-byte pieces of one row per thread (prefetch registers)

// the same row into registers (piece j of thread t = t + j * kBlock), stored to LDS after the current row's compute
__device__ __forceinline__ void dw_fetch_row(const uint16_t* __restrict__ src, uint2* v, int W, int C, int c0) {
#pragma unroll
  for (int j = 0; j < kPf; ++j) {
    const int i = threadIdx.x + j * kBlock, col = i / (kSlice / 4), q = i % (kSlice / 4);
    v[j] = make_uint2(0u, 0u);
    if (i < W * (kSlice / 4) && c0 + 4 * q < C) v[j] = *reinterpret_cast<const uint2*>(src + (size_t)col * C + c0 + 4 * q);
  }
}
__device__ __forceinline__ void dw_store_row(const uint2* v, uint16_t* __restrict__ dst, int W) {
#pragma unroll
  for (int j = 0; j < kPf; ++j) {
    const int i = threadIdx.x + j * kBlock;
    if (i < W * (kSlice / 4)) *reinterpret_cast<uint2*>(dst + (i / (kSlice / 4)) * kSlice + 4 * (i % (kSlice / 4))) = v[j];
  }
}

// grid (groups * strips, slices): part[blockIdx.x * slices + blockIdx.y] = [50][32] fp32 sums of this workgroup.  The next output
// row's new input row and dz row are fetched into registers before the current row is computed, so their latency hides behind it.
__global__ __launch_bounds__(kBlock) void k_dw_wgrad(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dz, float* __restrict__ part,
                                                     int n, int H, int W, int C, int strip_rows, int strips, int imgs_per_wg) {
  extern __shared__ uint16_t s_mem[];
  const int WP = W + 6;
  uint16_t* s_x = s_mem;                          // [7][W + 6][32], slot = (input row + 7) % 7
  uint16_t* s_dz = s_mem + 7 * WP * kSlice;       // [W][32]
  const int strip = blockIdx.x % strips, grp = blockIdx.x / strips;
  const int c0 = blockIdx.y * kSlice;
  const int h0 = strip * strip_rows, h1 = min(H, h0 + strip_rows);
  const int n0 = grp * imgs_per_wg, n1 = min(n, n0 + imgs_per_wg);
  for (int i = threadIdx.x; i < 7 * WP * kSlice / 2; i += kBlock) reinterpret_cast<uint32_t*>(s_x)[i] = 0u;   // padding columns stay 0
  const int cl = threadIdx.x % kSlice, dy = threadIdx.x / kSlice;                                          // dy 7: loads only
  float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float accb = 0.f;
  const size_t row_elems = (size_t)W * C;
  uint2 px[kPf], pd[kPf];
  for (int img = n0; img < n1; ++img) {
    const size_t img_off = (size_t)img * H * row_elems;
    for (int h = h0; h < h1; ++h) {
      __syncthreads();                            // the previous row's reads of the window and dz are done
      if (h == h0) {                              // a strip starts: its first 7 input rows and dz row, straight to LDS
        for (int r = h - 3; r <= h + 3; ++r)
          if (r >= 0 && r < H) dw_load_row(x + img_off + (size_t)r * row_elems, s_x + ((r + 7) % 7) * WP * kSlice + 3 * kSlice, W, C, c0);
        dw_load_row(dz + img_off + (size_t)h * row_elems, s_dz, W, C, c0);
      } else {                                    // the rows fetched during the previous row's compute
        if (h + 3 < H) dw_store_row(px, s_x + ((h + 3 + 7) % 7) * WP * kSlice + 3 * kSlice, W);
        dw_store_row(pd, s_dz, W);
      }
      __syncthreads();
      if (h + 1 < h1) {
        if (h + 4 < H) dw_fetch_row(x + img_off + (size_t)(h + 4) * row_elems, px, W, C, c0);
        dw_fetch_row(dz + img_off + (size_t)(h + 1) * row_elems, pd, W, C, c0);
      }
      const int r = h + dy - 3;
      if (dy < 7 && r >= 0 && r < H) {            // rows outside the image contribute nothing (their slots are stale, never read)
        const uint16_t* xr = s_x + ((r + 7) % 7) * WP * kSlice + cl;
        float win[7];
#pragma unroll
        for (int k = 0; k < 6; ++k) win[k] = bf2f(xr[k * kSlice]);
        for (int w = 0; w < W; ++w) {
          win[6] = bf2f(xr[(w + 6) * kSlice]);
          const float g = bf2f(s_dz[w * kSlice + cl]);
#pragma unroll
          for (int k = 0; k < 7; ++k) acc[k] = fmaf(win[k], g, acc[k]);
          if (dy == 3) accb += g;
#pragma unroll
          for (int k = 0; k < 6; ++k) win[k] = win[k + 1];
        }
      }
    }
  }
  float* p = part + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * kDwRows * kSlice;
  if (dy < 7) {
#pragma unroll
    for (int k = 0; k < 7; ++k) p[(dy * 7 + k) * kSlice + cl] = acc[k];
    if (dy == 3) p[kTaps * kSlice + cl] = accb;
  }
}

// out_a / out_b (+)= sum over the partial slots in a fixed order.  part: [n_part][slices][rows][32] -- row k < rows_a goes to out_a
// (layout 0: [rows_a][c], 1: [c][rows_a]), row rows_a to out_b (nullable).  One workgroup per (row, 32-channel slice): 8 threads per
// channel each add a contiguous eighth of the slots, then one thread adds the eight sums in segment order.
constexpr int kSeg = kBlock / kSlice;
__global__ __launch_bounds__(kBlock) void k_fold(const float* __restrict__ part, int n_part, int slices, int rows, int C, int rows_a,
                                                 float* __restrict__ out_a, int layout, float* __restrict__ out_b, int accumulate) {
  __shared__ float s_seg[kBlock];
  const int k = blockIdx.x / slices, sl = blockIdx.x % slices;
  if (k >= rows_a && !out_b) return;                                  // uniform over the workgroup
  const int cl = threadIdx.x % kSlice, seg = threadIdx.x / kSlice, c = sl * kSlice + cl;
  const size_t stride = (size_t)slices * rows * kSlice;
  const float* src = part + ((size_t)sl * rows + k) * kSlice + cl;
  const int per = (n_part + kSeg - 1) / kSeg, q0 = seg * per, q1 = min(n_part, q0 + per);
  float s = 0.f;
  for (int q = q0; q < q1; ++q) s += src[q * stride];
  s_seg[threadIdx.x] = s;
  __syncthreads();
  if (seg == 0 && c < C) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < kSeg; ++j) t += s_seg[j * kSlice + cl];
    float* o = k < rows_a ? out_a + (layout ? (size_t)c * rows_a + k : (size_t)k * C + c) : out_b + c;
    *o = accumulate ? *o + t : t;
  }
}

// layer-scale backward over a chunk of rows: dv = gamma * dx (bf16), partial sums of dx * u2 and of gamma * dx per channel.
// Thread (channel octet, row lane): rp rows in flight; the rp partial rows are folded in LDS in row-lane order.
__global__ __launch_bounds__(kBlock) void k_ls_bwd(const uint16_t* __restrict__ dx, const uint16_t* __restrict__ u2, const float* __restrict__ gamma,
                                                   uint16_t* __restrict__ dv, float* __restrict__ part, int rows, int C, int chunk) {
  __shared__ float s_g[2 * kBlock * 8];              // [2][rp][c], rp * c <= 8 * 256
  const int oc = C / 8, rp = kBlock / oc;
  float* s_b = s_g + rp * C;
  const int t = threadIdx.x, oct = t % oc, lane = t / oc;
  const int r0 = blockIdx.x * chunk, r1 = min(rows, r0 + chunk);
  float ag[8], ab[8], gm[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) ag[k] = ab[k] = 0.f;
  if (lane < rp) {
#pragma unroll
    for (int k = 0; k < 8; ++k) gm[k] = gamma[oct * 8 + k];
    for (int r = r0 + lane; r < r1; r += rp) {
      const size_t o = (size_t)r * C + oct * 8;
      const uint4 a = *reinterpret_cast<const uint4*>(dx + o), b = *reinterpret_cast<const uint4*>(u2 + o);
      const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
      uint32_t vw[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d0 = __uint_as_float(aw[j] << 16), d1 = __uint_as_float(aw[j] & 0xFFFF0000u);
        const float v0 = gm[2 * j] * d0, v1 = gm[2 * j + 1] * d1;
        ag[2 * j] = fmaf(d0, __uint_as_float(bw[j] << 16), ag[2 * j]);
        ag[2 * j + 1] = fmaf(d1, __uint_as_float(bw[j] & 0xFFFF0000u), ag[2 * j + 1]);
        ab[2 * j] += v0;
        ab[2 * j + 1] += v1;
        vw[j] = (uint32_t)f2bf(v0) | ((uint32_t)f2bf(v1) << 16);
      }
      *reinterpret_cast<uint4*>(dv + o) = make_uint4(vw[0], vw[1], vw[2], vw[3]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      s_g[lane * C + oct * 8 + k] = ag[k];
      s_b[lane * C + oct * 8 + k] = ab[k];
    }
  }
  __syncthreads();
  const int slices = (C + kSlice - 1) / kSlice;
  for (int c = t; c < C; c += kBlock) {
    float sg = 0.f, sb = 0.f;
    for (int l = 0; l < rp; ++l) {
      sg += s_g[l * C + c];
      sb += s_b[l * C + c];
    }
    float* p = part + ((size_t)blockIdx.x * slices + c / kSlice) * 2 * kSlice + c % kSlice;   // the [slices][2][32] layout k_fold reads
    p[0] = sg;
    p[kSlice] = sb;
  }
}

// x_out = x_in + gamma * u2, eight channels per thread (x_out may alias x_in)
__global__ __launch_bounds__(kBlock) void k_ls_fwd(const uint16_t* x_in, const uint16_t* __restrict__ u2, const float* __restrict__ gamma,
                                                   uint16_t* x_out, int C, size_t total8) {
  const int c8 = C / 8;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total8; i += (size_t)gridDim.x * kBlock) {
    const int c = (int)(i % c8) * 8;
    const uint4 a = reinterpret_cast<const uint4*>(x_in)[i], b = reinterpret_cast<const uint4*>(u2)[i];
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float y0 = fmaf(gamma[c + 2 * j], __uint_as_float(bw[j] << 16), __uint_as_float(aw[j] << 16));
      const float y1 = fmaf(gamma[c + 2 * j + 1], __uint_as_float(bw[j] & 0xFFFF0000u), __uint_as_float(aw[j] & 0xFFFF0000u));
      o[j] = (uint32_t)f2bf(y0) | ((uint32_t)f2bf(y1) << 16);
    }
    reinterpret_cast<uint4*>(x_out)[i] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

bool al(const void* p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

bool dw_shape_ok(int n, int h, int w, int c) {
  return n > 0 && n <= 65535 && h > 0 && h <= 65535 && w > 0 && w <= kMaxW && c > 0 && c % 8 == 0 && c <= 1024;
}

bool ls_shape_ok(long long rows, int c) { return rows > 0 && rows < (1ll << 31) && c > 0 && c % 8 == 0 && c <= 1024 && rows * c < (1ll << 40); }

int ls_chunk(int rows, int c) {
  const int rp = kBlock / (c / 8);
  int chunk = (rows + 255) / 256;                 // ~256 workgroups
  if (chunk < 16) chunk = 16;
  return (chunk + rp - 1) / rp * rp;
}

}  // namespace

size_t rart_cnx_dwconv_wgrad_workspace_bytes(int n, int h, int w, int c) {
  if (!dw_shape_ok(n, h, w, c)) return 0;
  const DwGeom g = dw_geom(n, h, c);
  return (size_t)g.groups * g.strips * g.slices * kDwRows * kSlice * sizeof(float);
}

int rart_cnx_dwconv_wgrad_bf16(const void* x, const void* dz, float* dw, float* db, int n, int h, int w, int c, int dw_layout, int accumulate,
                               void* workspace, size_t workspace_bytes, rart_stream_t stream) {
  RART_CHECK_ARG(x && dz && dw && db && workspace && (dw_layout == 0 || dw_layout == 1), "rart_cnx_dwconv_wgrad_bf16: bad arguments");
  RART_CHECK_ARG(al(x, 8) && al(dz, 8), "rart_cnx_dwconv_wgrad_bf16: x / dz 8-byte aligned");
  RART_CHECK_ARG(dw_shape_ok(n, h, w, c), "rart_cnx_dwconv_wgrad_bf16: c a multiple of 8, at most 1024; w <= %d; n, h <= 65535", kMaxW);
  RART_CHECK_ARG(workspace_bytes >= rart_cnx_dwconv_wgrad_workspace_bytes(n, h, w, c),
                 "rart_cnx_dwconv_wgrad_bf16: workspace smaller than rart_cnx_dwconv_wgrad_workspace_bytes");
  const DwGeom g = dw_geom(n, h, c);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)(7 * (w + 6) + w) * kSlice * sizeof(uint16_t);
  if (!rart_raise_dynamic_lds((const void*)k_dw_wgrad, lds, "rart_cnx_dwconv_wgrad_bf16")) return RART_ERR_HIP;
  hipLaunchKernelGGL(k_dw_wgrad, dim3(g.groups * g.strips, g.slices), dim3(kBlock), lds, st, (const uint16_t*)x, (const uint16_t*)dz,
                     (float*)workspace, n, h, w, c, g.strip_rows, g.strips, g.imgs_per_wg);
  RART_CHECK_LAUNCH("rart_cnx_dwconv_wgrad_bf16");
  hipLaunchKernelGGL(k_fold, dim3(kDwRows * g.slices), dim3(kBlock), 0, st, (const float*)workspace, g.groups * g.strips, g.slices,
                     kDwRows, c, kTaps, dw, dw_layout, db, accumulate);
  RART_CHECK_LAUNCH("rart_cnx_dwconv_wgrad_bf16 (fold)");
  return RART_OK;
}

size_t rart_cnx_layer_scale_bwd_workspace_bytes(long long rows, int c) {
  if (!ls_shape_ok(rows, c)) return 0;
  const int chunk = ls_chunk((int)rows, c);
  return (size_t)((rows + chunk - 1) / chunk) * ((c + kSlice - 1) / kSlice) * 2 * kSlice * sizeof(float);
}

int rart_cnx_layer_scale_bwd_bf16(const void* dx, const void* u2, const float* gamma, void* dv, float* dgamma, float* db2, long long rows,
                                  int c, int accumulate, void* workspace, size_t workspace_bytes, rart_stream_t stream) {
  RART_CHECK_ARG(dx && u2 && gamma && dv && dgamma && workspace && dv != dx && dv != u2, "rart_cnx_layer_scale_bwd_bf16: bad arguments "
                 "(dv must not alias dx or u2)");
  RART_CHECK_ARG(al(dx, 16) && al(u2, 16) && al(dv, 16), "rart_cnx_layer_scale_bwd_bf16: dx / u2 / dv 16-byte aligned");
  RART_CHECK_ARG(ls_shape_ok(rows, c), "rart_cnx_layer_scale_bwd_bf16: c a multiple of 8, at most 1024; 0 < rows < 2^31");
  RART_CHECK_ARG(workspace_bytes >= rart_cnx_layer_scale_bwd_workspace_bytes(rows, c),
                 "rart_cnx_layer_scale_bwd_bf16: workspace smaller than rart_cnx_layer_scale_bwd_workspace_bytes");
  const int chunk = ls_chunk((int)rows, c), n_part = (int)((rows + chunk - 1) / chunk), slices = (c + kSlice - 1) / kSlice;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ls_bwd, dim3(n_part), dim3(kBlock), 0, st, (const uint16_t*)dx, (const uint16_t*)u2, gamma, (uint16_t*)dv,
                     (float*)workspace, (int)rows, c, chunk);
  RART_CHECK_LAUNCH("rart_cnx_layer_scale_bwd_bf16");
  hipLaunchKernelGGL(k_fold, dim3(2 * slices), dim3(kBlock), 0, st, (const float*)workspace, n_part, slices, 2, c, 1, dgamma, 0, db2,
                     accumulate);
  RART_CHECK_LAUNCH("rart_cnx_layer_scale_bwd_bf16 (fold)");
  return RART_OK;
}

int rart_cnx_layer_scale_fwd_bf16(const void* x_in, const void* u2, const float* gamma, void* x_out, long long rows, int c, rart_stream_t stream) {
  RART_CHECK_ARG(x_in && u2 && gamma && x_out && x_out != u2, "rart_cnx_layer_scale_fwd_bf16: bad arguments (x_out must not alias u2)");
  RART_CHECK_ARG(al(x_in, 16) && al(u2, 16) && al(x_out, 16), "rart_cnx_layer_scale_fwd_bf16: x_in / u2 / x_out 16-byte aligned");
  RART_CHECK_ARG(ls_shape_ok(rows, c), "rart_cnx_layer_scale_fwd_bf16: c a multiple of 8, at most 1024; 0 < rows < 2^31");
  const size_t total8 = (size_t)rows * c / 8;
  hipLaunchKernelGGL(k_ls_fwd, dim3(rart_grid_for(total8, kBlock, 256 * 16)), dim3(kBlock), 0, (hipStream_t)stream, (const uint16_t*)x_in,
                     (const uint16_t*)u2, gamma, (uint16_t*)x_out, c, total8);
  RART_CHECK_LAUNCH("rart_cnx_layer_scale_fwd_bf16");
  return RART_OK;
}
