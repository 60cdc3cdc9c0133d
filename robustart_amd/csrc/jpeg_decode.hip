// JPEG reader for gfx950: Image.open(f).convert('RGB') of a batch of baseline files, bit-exact with Pillow / libjpeg-turbo.
// Reference: the 'pil' decoder of RobustART/noise/utils/imagenet_s_gen.py:177-196 and the file reader behind
// exprs/nips_benchmark/pgd_adv_train/resnet50/config.yaml:38-56; arithmetic: jidctint.c, jdsample.c, jdcolor.c.
//
// Host: rart_jpeg_probe / rart_jpeg_entropy_decode (jpeg_entropy.h) turn file bytes into int16 coefficient blocks.
// Device, two launches per batch whatever its size or mix of image sizes and samplings:
//   k_jpeg_idct  : one thread per 8x8 block over the batch's global block numbering.  A workgroup's 256 blocks (32 KiB of
//                  coefficients) are staged through LDS with one 16-byte load per lane, contiguous across the wave; each thread
//                  then reads its block back (144-byte pitch: conflict-free 16-byte LDS reads), dequantises, runs the ISLOW
//                  IDCT in registers and writes 8 rows of 8 bytes to its component plane (neighbouring lanes = neighbouring
//                  blocks of a block row = contiguous bytes).
//   k_jpeg_color : one thread per output pixel: libjpeg's upsampling of the two chroma planes + YCbCr -> RGB, packed u8.
// Both find their image by bisection over the descriptor table (block_start / out_off are ascending).
#include "rart_common.h"
#include "jpeg_entropy.h"
#include "jpeg_idct.h"

namespace {
constexpr int kThreads = 256;
constexpr int kPitch = 9;   // uint4 per staged block: 8 of coefficients + 1 of padding

constexpr int FIXC(double x) { return (int)(x * 65536.0 + 0.5); }

__global__ __launch_bounds__(kThreads) void k_jpeg_idct(const rart_jpeg_desc* __restrict__ desc, int n,
                                                        const int16_t* __restrict__ coef, long long total_blocks,
                                                        const uint16_t* __restrict__ qt, uint8_t* __restrict__ ws) {
  __shared__ uint4 stage[kThreads * kPitch];
  const long long g0 = (long long)blockIdx.x * kThreads;
  const long long left = total_blocks - g0;
  const int chunks = (int)(left < kThreads ? left : kThreads) * 8;
  const uint4* src = reinterpret_cast<const uint4*>(coef) + g0 * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = threadIdx.x + j * kThreads;
    if (i < chunks) stage[(i >> 3) * kPitch + (i & 7)] = src[i];
  }
  __syncthreads();
  const long long g = g0 + threadIdx.x;
  if (g >= total_blocks) return;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid].block_start[0] <= g) lo = mid; else hi = mid - 1;
  }
  const rart_jpeg_desc& d = desc[lo];
  const int c = g >= d.block_start[2] ? 2 : (g >= d.block_start[1] ? 1 : 0);
  const int local = (int)(g - d.block_start[c]);
  const int bw = d.blocks_w[c];
  const int by = local / bw, bx = local - by * bw;
  const uint4* q = reinterpret_cast<const uint4*>(qt + d.qt_off + c * 64);
  int b[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 v = stage[threadIdx.x * kPitch + r];
    const uint4 t = q[r];
    const uint32_t vw[4] = {v.x, v.y, v.z, v.w}, tw[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      b[r * 8 + 2 * k] = (int)(int16_t)(vw[k] & 0xFFFFu) * (int)(tw[k] & 0xFFFFu);
      b[r * 8 + 2 * k + 1] = (int)(int16_t)(vw[k] >> 16) * (int)(tw[k] >> 16);
    }
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) idct8<11>(b + col, 8);
#pragma unroll
  for (int r = 0; r < 8; ++r) idct8<18>(b + r * 8, 1);
  const int stride = bw * 8;
  uint8_t* p = ws + d.plane_off[c] + (size_t)by * 8 * stride + bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    uint32_t w0 = 0, w1 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int v0 = b[r * 8 + k] + 128, v1 = b[r * 8 + 4 + k] + 128;
      v0 = v0 < 0 ? 0 : (v0 > 255 ? 255 : v0);
      v1 = v1 < 0 ? 0 : (v1 > 255 ? 255 : v1);
      w0 |= (uint32_t)v0 << (8 * k);
      w1 |= (uint32_t)v1 << (8 * k);
    }
    *reinterpret_cast<uint2*>(p + (size_t)r * stride) = make_uint2(w0, w1);   // plane_off % 16 == 0, stride % 8 == 0
  }
}

// one chroma sample of output pixel (y, x): jdsample.c's h2v1 / h2v2 fancy (triangle) filters, plain replication when the plane is
// at most two samples wide, the plane itself at 4:4:4; dw x dh is the component's real extent, indices never leave it
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ pl, int stride, int dw, int dh, int hs, int vs, int y, int x) {
  if (hs == 1) return pl[(size_t)y * stride + x];
  const int i = x >> 1;
  if (dw <= 2) return pl[(size_t)(vs == 2 ? y >> 1 : y) * stride + i];
  const int il = i > 0 ? i - 1 : 0, ir = i < dw - 1 ? i + 1 : dw - 1;
  if (vs == 1) {
    const uint8_t* row = pl + (size_t)y * stride;
    const int v = row[i];
    if (x & 1) return i == dw - 1 ? v : (3 * v + row[ir] + 2) >> 2;
    return i == 0 ? v : (3 * v + row[il] + 1) >> 2;
  }
  const int cy = y >> 1;
  const int far = (y & 1) ? (cy < dh - 1 ? cy + 1 : dh - 1) : (cy > 0 ? cy - 1 : 0);
  const uint8_t* rn = pl + (size_t)cy * stride;
  const uint8_t* rf = pl + (size_t)far * stride;
  const int cs = 3 * rn[i] + rf[i];
  if (x & 1) return i == dw - 1 ? (4 * cs + 7) >> 4 : (3 * cs + 3 * rn[ir] + rf[ir] + 7) >> 4;
  return i == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * rn[il] + rf[il] + 8) >> 4;
}

__global__ __launch_bounds__(kThreads) void k_jpeg_color(const rart_jpeg_desc* __restrict__ desc, int n,
                                                         const uint8_t* __restrict__ ws, uint8_t* __restrict__ out,
                                                         long long total_pixels) {
  constexpr int H = 32768;
  const long long step = (long long)gridDim.x * kThreads;
  for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < total_pixels; p += step) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (desc[mid].out_off <= 3 * p) lo = mid; else hi = mid - 1;
    }
    const rart_jpeg_desc& d = desc[lo];
    const int w = d.width, h = d.height;
    const int local = (int)(p - d.out_off / 3);
    const int y = local / w, x = local - y * w;
    const int yy = ws[d.plane_off[0] + (size_t)y * (d.blocks_w[0] * 8) + x];
    uint8_t* o = out + 3 * p;
    if (d.ncomp == 1) {
      o[0] = o[1] = o[2] = (uint8_t)yy;
      continue;
    }
    const int hs = d.h_samp, vs = d.v_samp;
    const int dw = (w + hs - 1) / hs, dh = (h + vs - 1) / vs;
    const int vb = chroma_at(ws + d.plane_off[1], d.blocks_w[1] * 8, dw, dh, hs, vs, y, x) - 128;
    const int vr = chroma_at(ws + d.plane_off[2], d.blocks_w[2] * 8, dw, dh, hs, vs, y, x) - 128;
    int r = yy + ((FIXC(1.40200) * vr + H) >> 16);
    int b = yy + ((FIXC(1.77200) * vb + H) >> 16);
    int g = yy + ((-FIXC(0.34414) * vb + H - FIXC(0.71414) * vr) >> 16);
    r = r < 0 ? 0 : (r > 255 ? 255 : r);
    g = g < 0 ? 0 : (g > 255 ? 255 : g);
    b = b < 0 ? 0 : (b > 255 ? 255 : b);
    o[0] = (uint8_t)r;
    o[1] = (uint8_t)g;
    o[2] = (uint8_t)b;
  }
}

// The host copy of the descriptor table against the caller's buffer sizes; `need_ws` receives the workspace bytes the planes span.
int check_descs(const rart_jpeg_desc* d, int n, long long total_blocks, size_t qt_count, size_t out_bytes, size_t* need_ws,
                long long* total_pixels) {
  long long blk = 0, pix = 0;
  size_t ws = 0;
  for (int i = 0; i < n; ++i) {
    const rart_jpeg_desc& e = d[i];
    RART_CHECK_ARG(e.ncomp == 1 || e.ncomp == 3, "rart_jpeg_decode_u8: descriptor %d: ncomp must be 1 or 3", i);
    RART_CHECK_ARG(e.height >= 1 && e.width >= 1 && e.height <= 65535 && e.width <= 65535 &&
                       (long long)e.height * e.width <= rart_jpeg::kMaxPixels,
                   "rart_jpeg_decode_u8: descriptor %d: image size out of range", i);
    const bool samp_ok = e.ncomp == 1 ? (e.h_samp == 1 && e.v_samp == 1)
                                      : ((e.h_samp == 1 || e.h_samp == 2) && (e.v_samp == 1 || e.v_samp == 2) && e.h_samp >= e.v_samp);
    RART_CHECK_ARG(samp_ok, "rart_jpeg_decode_u8: descriptor %d: luma sampling must be (1,1), (2,1) or (2,2)", i);
    const int mcux = (e.width + 8 * e.h_samp - 1) / (8 * e.h_samp), mcuy = (e.height + 8 * e.v_samp - 1) / (8 * e.v_samp);
    for (int c = 0; c < 3; ++c) {
      const int bw = c < e.ncomp ? (c == 0 ? mcux * e.h_samp : mcux) : 0, bh = c < e.ncomp ? (c == 0 ? mcuy * e.v_samp : mcuy) : 0;
      RART_CHECK_ARG(e.blocks_w[c] == bw && e.blocks_h[c] == bh, "rart_jpeg_decode_u8: descriptor %d: block grid of component %d", i, c);
      RART_CHECK_ARG(e.block_start[c] == blk, "rart_jpeg_decode_u8: descriptor %d: block_start[%d] must continue the numbering", i, c);
      blk += (long long)bw * bh;
      if (c < e.ncomp) {
        const size_t bytes = (size_t)bw * bh * 64;
        RART_CHECK_ARG(e.plane_off[c] >= 0 && e.plane_off[c] % 16 == 0, "rart_jpeg_decode_u8: descriptor %d: plane_off[%d] alignment", i, c);
        if ((size_t)e.plane_off[c] + bytes > ws) ws = (size_t)e.plane_off[c] + bytes;
      }
    }
    RART_CHECK_ARG(e.qt_off >= 0 && e.qt_off % 8 == 0 && (size_t)e.qt_off + 192 <= qt_count,
                   "rart_jpeg_decode_u8: descriptor %d: quantisation tables outside qt", i);
    RART_CHECK_ARG(e.out_off == 3 * pix, "rart_jpeg_decode_u8: descriptor %d: out_off must pack the images back to back", i);
    pix += (long long)e.height * e.width;
  }
  RART_CHECK_ARG(blk == total_blocks, "rart_jpeg_decode_u8: the descriptors hold %lld blocks, total_blocks says %lld", blk, total_blocks);
  if ((size_t)(3 * pix) > out_bytes) {
    rart_set_error("rart_jpeg_decode_u8: out of %zu bytes required, got %zu", (size_t)(3 * pix), out_bytes);
    return RART_ERR_INVALID;
  }
  *need_ws = rart_align_up(ws, 256);
  *total_pixels = pix;
  return RART_OK;
}
}  // namespace

extern "C" {

int rart_jpeg_probe(const uint8_t* data_host, size_t len, rart_jpeg_info* info_host) {
  const rart_jpeg::Result r = rart_jpeg::probe(data_host, len, info_host);
  if (r.status != RART_OK) rart_set_error("rart_jpeg_probe: %s", r.why);
  return r.status;
}

int rart_jpeg_entropy_decode(const uint8_t* data_host, size_t len, const rart_jpeg_info* info_host, int16_t* coef_host,
                             size_t capacity) {
  const rart_jpeg::Result r = rart_jpeg::entropy_decode(data_host, len, info_host, coef_host, capacity);
  if (r.status != RART_OK) rart_set_error("rart_jpeg_entropy_decode: %s", r.why);
  return r.status;
}

size_t rart_jpeg_decode_workspace_bytes(const rart_jpeg_desc* desc_host, int n) {
  if (!desc_host || n <= 0) return 0;
  size_t ws = 0;
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 3 && c < desc_host[i].ncomp; ++c) {
      if (desc_host[i].plane_off[c] < 0 || desc_host[i].blocks_w[c] < 0 || desc_host[i].blocks_h[c] < 0) return 0;
      const size_t end = (size_t)desc_host[i].plane_off[c] + (size_t)desc_host[i].blocks_w[c] * desc_host[i].blocks_h[c] * 64;
      if (end > ws) ws = end;
    }
  return rart_align_up(ws, 256);
}

int rart_jpeg_decode_u8(const rart_jpeg_desc* desc, const rart_jpeg_desc* desc_host, int n, const int16_t* coef, int64_t total_blocks,
                        const uint16_t* qt, size_t qt_count, void* workspace, size_t workspace_bytes, uint8_t* out, size_t out_bytes,
                        rart_stream_t stream) {
  RART_CHECK_ARG(n > 0, "rart_jpeg_decode_u8: descriptor count must be positive, got %d", n);
  RART_CHECK_ARG(desc && desc_host && coef && qt && out && total_blocks > 0, "rart_jpeg_decode_u8: bad arguments");
  RART_CHECK_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)qt & 15) == 0 && ((uintptr_t)desc & 7) == 0 && ((uintptr_t)workspace & 15) == 0,
                 "rart_jpeg_decode_u8: coef, qt and the workspace must be 16-byte aligned, desc 8-byte aligned");
  size_t need = 0;
  long long pixels = 0;
  const int st = check_descs(desc_host, n, total_blocks, qt_count, out_bytes, &need, &pixels);
  if (st != RART_OK) return st;
  if (!workspace || workspace_bytes < need) {
    rart_set_error("rart_jpeg_decode_u8: workspace of %zu bytes required, got %zu", need, workspace_bytes);
    return RART_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const long long grid = (total_blocks + kThreads - 1) / kThreads;
  RART_CHECK_ARG(grid <= 0x7FFFFFFFll, "rart_jpeg_decode_u8: too many blocks for one launch");
  hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)grid), dim3(kThreads), 0, s, desc, n, coef, (long long)total_blocks, qt,
                     (uint8_t*)workspace);
  RART_CHECK_LAUNCH("rart_jpeg_decode_u8 (idct)");
  hipLaunchKernelGGL(k_jpeg_color, dim3(rart_grid_for((size_t)pixels, kThreads, 256 * 16)), dim3(kThreads), 0, s, desc, n,
                     (const uint8_t*)workspace, out, pixels);
  RART_CHECK_LAUNCH("rart_jpeg_decode_u8 (colour)");
  return RART_OK;
}

}  // extern "C"
