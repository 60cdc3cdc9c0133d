// Batched variable-size resize on gfx950: Pillow's Image.resize for 8-bit RGB for n images of different sizes in one call,
// bit-exact: crop(box) -> resize -> crop window -> mirror (imagenet_s_gen.py:119-120, torchvision's resized_crop).
// Arithmetic: resize_pil.hip's (22-bit fixed-point coefficients from resize_pil_tables.h, one pass to a uint8 intermediate, then
// the other), plus two things Pillow does that the single-size entry does not restate:
//   - pass order: Image.resize runs the vertical pass first when the source is more than 100 times as tall as wide and the
//     height shrinks (PIL/Image.py, resize()); the intermediate's rounding makes the two orders differ, so each descriptor
//     carries the order (`vfirst`);
//   - NEAREST is Geometry.c's ImagingScaleAffine: the source column / row of every output column / row comes from a double
//     accumulated on the host (xo += scale), as Pillow builds its xintab, stored as an index table -- a 16.16 walk picks the
//     neighbouring pixel where a centre falls exactly on a pixel boundary (1000 -> 36 columns).
// Shape: jpeg_decode.hip's --
//   rart_resize_batch_plan (host only) writes header | descriptors | prefix table | coefficient tables into one host buffer, which
//   crosses the bus in one copy; rart_resize_batch_u8 validates the host copy, then launches
//   k_batch_pass1 : one thread per sample of the intermediate.  Image i has mid_count_i * crop_w * 3 of them (horizontal pass
//               first: mid_count rows, which follow its vertical scale) or crop_h * mid_count_i * 3 (vertical first: mid_count
//               columns), numbered image by image; a thread finds its image by bisection over the prefix table.
//   k_batch_pass2 : one thread per output sample; every image has crop_h * crop_w * 3, so the image is a division.  The mirror
//               is the column the thread writes to.
//   k_batch_nearest : one thread per output pixel (NEAREST only; index tables, no intermediate).
// Every index a kernel forms is bounded by a value rart_resize_batch_u8 has checked on the host copy.
#include "rart_common.h"
#include "resize_pil_tables.h"
#include <string.h>

namespace {
using namespace rart_pil;
constexpr int kBlock = 256;
constexpr int kMaxSide = 65535;

static_assert(sizeof(rart_resize_desc) == 64 && sizeof(rart_resize_plan) == 80, "layout documented in robustart_hip.h");

__device__ __forceinline__ uint8_t clip8(int acc) {
  acc >>= 22;
  return (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

// acc over `cnt` taps `stride` bytes apart
__device__ __forceinline__ uint8_t taps(const uint8_t* __restrict__ src, size_t stride, const int* __restrict__ k, int cnt) {
  int acc = 1 << 21;
  for (int j = 0; j < cnt; ++j) acc += (int)src[(size_t)j * stride] * k[j];
  return clip8(acc);
}

__global__ __launch_bounds__(kBlock) void k_batch_pass1(const rart_resize_desc* __restrict__ desc, const long long* __restrict__ prefix,
                                                        const int* __restrict__ tabs, int n, int cy, int cx, int cw,
                                                        uint8_t* __restrict__ tmp) {
  const long long total = prefix[n];
  const long long step = (long long)gridDim.x * kBlock;
  for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < total; g += step) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (prefix[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const rart_resize_desc& d = desc[lo];
    const int local = (int)(g - prefix[lo]);          // < the image's items, checked to fit an int
    const int p = local / 3, c = local - p * 3;
    const uint8_t* img = reinterpret_cast<const uint8_t*>(d.src) + ((size_t)d.box_y * d.w + d.box_x) * 3 + c;
    if (!d.vfirst) {                                  // tmp[mid_count][cw][3]: rows mid_first.. of the box, the crop's columns
      const int yo = p / cw, xo = p - yo * cw;
      const int* row = tabs + d.tab_h + (size_t)(cx + xo) * (d.ks_h + 2);
      tmp[g] = taps(img + ((size_t)(d.mid_first + yo) * d.w + row[0]) * 3, 3, row + 2, row[1]);
    } else {                                          // tmp[ch][mid_count][3]: the crop's rows, columns mid_first.. of the box
      const int yo = p / d.mid_count, xo = p - yo * d.mid_count;
      const int* row = tabs + d.tab_v + (size_t)(cy + yo) * (d.ks_v + 2);
      tmp[g] = taps(img + ((size_t)row[0] * d.w + (d.mid_first + xo)) * 3, (size_t)d.w * 3, row + 2, row[1]);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_batch_pass2(const rart_resize_desc* __restrict__ desc, const long long* __restrict__ prefix,
                                                        const int* __restrict__ tabs, int n, int cy, int cx, int ch, int cw,
                                                        const uint8_t* __restrict__ tmp, uint8_t* __restrict__ out) {
  const int row3 = cw * 3;
  const long long total = (long long)n * ch * row3;
  const long long step = (long long)gridDim.x * kBlock;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += step) {
    const long long p = i / row3;
    const int col = (int)(i - p * row3);
    const int img = (int)(p / ch), yo = (int)(p - (long long)img * ch);
    const rart_resize_desc& d = desc[img];
    const int xo = col / 3, c = col - xo * 3;
    const uint8_t* mid = tmp + prefix[img];
    uint8_t v;
    if (!d.vfirst) {
      const int* row = tabs + d.tab_v + (size_t)(cy + yo) * (d.ks_v + 2);
      v = taps(mid + (size_t)(row[0] - d.mid_first) * row3 + col, row3, row + 2, row[1]);
    } else {
      const int* row = tabs + d.tab_h + (size_t)(cx + xo) * (d.ks_h + 2);
      v = taps(mid + ((size_t)yo * d.mid_count + (row[0] - d.mid_first)) * 3 + c, 3, row + 2, row[1]);
    }
    const int ox = d.flip ? cw - 1 - xo : xo;
    out[p * row3 + ox * 3 + c] = v;
  }
}

__global__ __launch_bounds__(kBlock) void k_batch_nearest(const rart_resize_desc* __restrict__ desc, const int* __restrict__ tabs, int n,
                                                          int cy, int cx, int ch, int cw, uint8_t* __restrict__ out) {
  const long long total = (long long)n * ch * cw;
  const long long step = (long long)gridDim.x * kBlock;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += step) {
    const long long p = i / cw;
    const int xo = (int)(i - p * cw);
    const int img = (int)(p / ch), yo = (int)(p - (long long)img * ch);
    const rart_resize_desc& d = desc[img];
    const int sx = tabs[d.tab_h + cx + xo], sy = tabs[d.tab_v + cy + yo];      // inside the box: checked on the host copy
    const uint8_t* s = reinterpret_cast<const uint8_t*>(d.src) + ((size_t)(d.box_y + sy) * d.w + (d.box_x + sx)) * 3;
    const int ox = d.flip ? cw - 1 - xo : xo;
    uint8_t* o = out + (p * cw + ox) * 3;
    o[0] = s[0];
    o[1] = s[1];
    o[2] = s[2];
  }
}

// the four regions behind one another, each 16-byte aligned
void layout(rart_resize_plan* p) {
  p->desc_off = (int64_t)rart_align_up(sizeof(rart_resize_plan), 16);
  p->prefix_off = p->desc_off + (int64_t)rart_align_up((size_t)p->n * sizeof(rart_resize_desc), 16);
  p->table_off = p->prefix_off + (int64_t)rart_align_up(((size_t)p->n + 1) * sizeof(long long), 16);
  p->total_bytes = p->table_off + p->table_count * (int64_t)sizeof(int);
}

// the per-call arguments and the caller's fields of one descriptor; `who` names the entry in the message
int check_call(const char* who, int n, int f, int rh, int rw, int cy, int cx, int ch, int cw) {
  RART_CHECK_ARG(n > 0, "%s: image count must be positive, got %d", who, n);
  RART_CHECK_ARG(f >= 0 && f <= 5, "%s: filter must be 0..5 (nearest, bilinear, bicubic, box, hamming, lanczos), got %d", who, f);
  RART_CHECK_ARG(rh > 0 && rw > 0 && rh <= kMaxSide && rw <= kMaxSide, "%s: target size %d x %d out of range", who, rh, rw);
  RART_CHECK_ARG(cy >= 0 && cx >= 0 && ch > 0 && cw > 0 && cy <= rh - ch && cx <= rw - cw,
                 "%s: crop window (%d, %d, %d, %d) outside the resized image %d x %d", who, cy, cx, ch, cw, rh, rw);
  return RART_OK;
}
int check_image(const char* who, int i, const rart_resize_desc& e) {
  RART_CHECK_ARG(e.src != 0, "%s: image %d: null source", who, i);
  RART_CHECK_ARG(e.h > 0 && e.w > 0 && e.h <= kMaxSide && e.w <= kMaxSide, "%s: image %d: size %d x %d out of range", who, i, e.h, e.w);
  RART_CHECK_ARG(e.box_y >= 0 && e.box_x >= 0 && e.box_h > 0 && e.box_w > 0 && e.box_y <= e.h - e.box_h && e.box_x <= e.w - e.box_w,
                 "%s: image %d: box (%d, %d, %d, %d) outside the image %d x %d", who, i, e.box_y, e.box_x, e.box_h, e.box_w, e.h, e.w);
  return RART_OK;
}

// one table of the host copy: rows [first, first + count) must lie in the table region and tap inside [lo, hi)
int check_table(const int* tabs, int64_t table_count, int off, int ks, int rows, int first, int count, int lo, int hi, int i,
                const char* which) {
  RART_CHECK_ARG(ks >= 1 && off >= 0 && (int64_t)off + (int64_t)rows * (ks + 2) <= table_count,
                 "rart_resize_batch_u8: image %d: %s table offset %d (%d rows of %d taps) outside the table region of %lld", i, which,
                 off, rows, ks, (long long)table_count);
  for (int r = first; r < first + count; ++r) {
    const int* row = tabs + off + (size_t)r * (ks + 2);
    RART_CHECK_ARG(row[1] >= 0 && row[1] <= ks && row[0] >= lo && row[0] <= hi - row[1],
                   "rart_resize_batch_u8: image %d: %s table row %d taps [%d, +%d) outside [%d, %d)", i, which, r, row[0], row[1], lo, hi);
  }
  return RART_OK;
}
// NEAREST's index table of the host copy: entries [first, first + count) must lie in the table region and point inside [0, size)
int check_index(const int* tabs, int64_t table_count, int off, int rows, int first, int count, int size, int i, const char* which) {
  RART_CHECK_ARG(off >= 0 && (int64_t)off + rows <= table_count,
                 "rart_resize_batch_u8: image %d: %s table offset %d (%d entries) outside the table region of %lld", i, which, off, rows,
                 (long long)table_count);
  for (int r = first; r < first + count; ++r)
    RART_CHECK_ARG(tabs[off + r] >= 0 && tabs[off + r] < size, "rart_resize_batch_u8: image %d: %s table entry %d = %d outside [0, %d)",
                   i, which, r, tabs[off + r], size);
  return RART_OK;
}
}  // namespace

extern "C" {

int rart_resize_batch_plan(const rart_resize_desc* images_host, int n, int filter, int resize_h, int resize_w, int crop_y, int crop_x,
                           int crop_h, int crop_w, void* plan_host, size_t capacity, rart_resize_plan* sizes) {
  static const char* who = "rart_resize_batch_plan";
  int st = check_call(who, n, filter, resize_h, resize_w, crop_y, crop_x, crop_h, crop_w);
  if (st != RART_OK) return st;
  RART_CHECK_ARG(images_host && (plan_host || sizes), "%s: bad arguments", who);
  RART_CHECK_ARG(((uintptr_t)plan_host & 15) == 0, "%s: plan_host must be 16-byte aligned", who);
  for (int i = 0; i < n; ++i)
    if ((st = check_image(who, i, images_host[i])) != RART_OK) return st;
  rart_resize_plan hd{};
  hd.n = n, hd.filter = filter, hd.resize_h = resize_h, hd.resize_w = resize_w;
  hd.crop_y = crop_y, hd.crop_x = crop_x, hd.crop_h = crop_h, hd.crop_w = crop_w;
  // the distinct tables of the call: (in_size, out_size) -> element of the table region
  std::map<std::pair<int, int>, std::pair<int, const CoeffTable*>> used;
  std::vector<const CoeffTable*> order;
  std::vector<CoeffTable> nearest;      // NEAREST: built per call (out_size ints each), not cached
  nearest.reserve(2 * (size_t)n);       // `order` keeps pointers into it
  auto table = [&](int in_size, int out_size) -> std::pair<int, const CoeffTable*> {
    auto it = used.find({in_size, out_size});
    if (it != used.end()) return it->second;
    const CoeffTable* t;
    if (filter == 0) {
      // Geometry.c ImagingScaleAffine with a = (in / out, 0, 0): xo = a * 0.5; xintab[x] = (int)xo; xo += a
      CoeffTable nt;
      nt.ksize = 0;
      nt.data.resize((size_t)out_size);
      const double a = (double)in_size / (double)out_size;
      double xo = a * 0.5;
      for (int x = 0; x < out_size; ++x, xo += a) {
        const int xin = xo < 0.0 ? -1 : (int)xo;
        nt.data[x] = xin > in_size - 1 ? in_size - 1 : xin;
      }
      nearest.push_back(std::move(nt));
      t = &nearest.back();
    } else {
      t = &coeff_table(in_size, out_size, filter);
    }
    const std::pair<int, const CoeffTable*> v{(int)hd.table_count, t};
    hd.table_count += (int64_t)t->data.size();
    order.push_back(t);
    used[{in_size, out_size}] = v;
    return v;
  };
  std::vector<rart_resize_desc> descs(images_host, images_host + n);
  std::vector<long long> prefix((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) {
    rart_resize_desc& d = descs[i];
    d.mid_first = d.mid_count = d.tab_h = d.ks_h = d.tab_v = d.ks_v = d.vfirst = 0;
    d.flip = d.flip ? 1 : 0;
    RART_CHECK_ARG(hd.table_count <= 0x3FFFFFFF, "%s: the call's coefficient tables exceed 2^30 entries", who);
    const auto th = table(d.box_w, resize_w), tv = table(d.box_h, resize_h);
    d.tab_h = th.first, d.ks_h = th.second->ksize, d.tab_v = tv.first, d.ks_v = tv.second->ksize;
    if (filter == 0) continue;          // no intermediate: prefix stays 0
    // PIL/Image.py resize(): `if self.size[1] > self.size[0] * 100 and size[1] < self.size[1]` -> vertical pass first
    d.vfirst = (long long)d.box_h > 100ll * d.box_w && resize_h < d.box_h;
    // the rows (columns, vertical first) of the box that the second pass reads through its taps over the crop window
    const CoeffTable* t2 = d.vfirst ? th.second : tv.second;
    const int lo = d.vfirst ? crop_x : crop_y, cnt = d.vfirst ? crop_w : crop_h;
    int first = d.vfirst ? d.box_w : d.box_h, last = 0;
    for (int r = lo; r < lo + cnt; ++r) {
      const int* row = &t2->data[(size_t)r * (t2->ksize + 2)];
      if (row[0] < first) first = row[0];
      if (row[0] + row[1] > last) last = row[0] + row[1];
    }
    d.mid_first = first, d.mid_count = last - first;
    prefix[i + 1] = prefix[i] + (long long)d.mid_count * (d.vfirst ? crop_h : crop_w) * 3;
  }
  RART_CHECK_ARG(hd.table_count <= 0x3FFFFFFF, "%s: the call's coefficient tables exceed 2^30 entries", who);
  hd.workspace_bytes = (int64_t)rart_align_up((size_t)prefix[n], 256);
  layout(&hd);
  if (sizes) *sizes = hd;
  if (!plan_host) return RART_OK;
  if (capacity < (size_t)hd.total_bytes) {
    rart_set_error("%s: plan buffer of %zu bytes required, got %zu", who, (size_t)hd.total_bytes, capacity);
    return RART_ERR_WORKSPACE;
  }
  uint8_t* base = (uint8_t*)plan_host;
  memset(base, 0, (size_t)hd.table_off);      // the alignment gaps too: the buffer is compared and copied as a whole
  memcpy(base, &hd, sizeof(hd));
  memcpy(base + hd.desc_off, descs.data(), (size_t)n * sizeof(rart_resize_desc));
  memcpy(base + hd.prefix_off, prefix.data(), ((size_t)n + 1) * sizeof(long long));
  int* tabs = (int*)(base + hd.table_off);
  for (const CoeffTable* t : order) {
    memcpy(tabs, t->data.data(), t->data.size() * sizeof(int));
    tabs += t->data.size();
  }
  return RART_OK;
}

int rart_resize_batch_u8(const void* plan, const void* plan_host, size_t plan_bytes, void* workspace, size_t workspace_bytes,
                         uint8_t* out, size_t out_bytes, rart_stream_t stream) {
  static const char* who = "rart_resize_batch_u8";
  RART_CHECK_ARG(plan && plan_host && out, "%s: bad arguments", who);
  RART_CHECK_ARG(((uintptr_t)plan & 15) == 0 && ((uintptr_t)plan_host & 7) == 0, "%s: the plan must be 16-byte aligned", who);
  RART_CHECK_ARG(plan_bytes >= sizeof(rart_resize_plan), "%s: plan of %zu bytes is shorter than its header", who, plan_bytes);
  const uint8_t* hb = (const uint8_t*)plan_host;
  rart_resize_plan hd;
  memcpy(&hd, hb, sizeof(hd));
  int st = check_call(who, hd.n, hd.filter, hd.resize_h, hd.resize_w, hd.crop_y, hd.crop_x, hd.crop_h, hd.crop_w);
  if (st != RART_OK) return st;
  RART_CHECK_ARG(hd.table_count >= 0 && hd.table_count <= 0x3FFFFFFF, "%s: table_count %lld out of range", who, (long long)hd.table_count);
  rart_resize_plan want = hd;
  layout(&want);
  RART_CHECK_ARG(want.desc_off == hd.desc_off && want.prefix_off == hd.prefix_off && want.table_off == hd.table_off &&
                     want.total_bytes == hd.total_bytes, "%s: the header's region offsets do not match its counts", who);
  RART_CHECK_ARG((size_t)hd.total_bytes <= plan_bytes, "%s: the plan holds %lld bytes, plan_bytes says %zu", who,
                 (long long)hd.total_bytes, plan_bytes);
  const rart_resize_desc* d = (const rart_resize_desc*)(hb + hd.desc_off);
  const long long* prefix = (const long long*)(hb + hd.prefix_off);
  const int* tabs = (const int*)(hb + hd.table_off);
  const int n = hd.n, cw = hd.crop_w, ch = hd.crop_h;
  RART_CHECK_ARG(prefix[0] == 0, "%s: the prefix table must start at 0", who);
  for (int i = 0; i < n; ++i) {
    const rart_resize_desc& e = d[i];
    if ((st = check_image(who, i, e)) != RART_OK) return st;
    if (hd.filter == 0) {
      RART_CHECK_ARG(prefix[i + 1] == 0, "%s: image %d: NEAREST has no horizontal-pass work", who, i);
      if ((st = check_index(tabs, hd.table_count, e.tab_h, hd.resize_w, hd.crop_x, cw, e.box_w, i, "column")) != RART_OK ||
          (st = check_index(tabs, hd.table_count, e.tab_v, hd.resize_h, hd.crop_y, ch, e.box_h, i, "row")) != RART_OK)
        return st;
      continue;
    }
    const bool vf = e.vfirst != 0;
    const int side = vf ? e.box_w : e.box_h;
    RART_CHECK_ARG(e.mid_first >= 0 && e.mid_count >= 1 && e.mid_first <= side - e.mid_count,
                   "%s: image %d: intermediate range [%d, +%d) outside the box's %d %s", who, i, e.mid_first, e.mid_count, side,
                   vf ? "columns" : "rows");
    const long long items = (long long)e.mid_count * (vf ? ch : cw) * 3;
    RART_CHECK_ARG(items <= 0x7FFFFFFF && prefix[i + 1] - prefix[i] == items,
                   "%s: image %d: the prefix table must continue the numbering by the image's %lld first-pass items", who, i, items);
    // the pass that reads the source taps inside the box; the pass that reads the intermediate taps inside [mid_first, +mid_count)
    const int h_lo = vf ? e.mid_first : 0, h_hi = vf ? e.mid_first + e.mid_count : e.box_w;
    const int v_lo = vf ? 0 : e.mid_first, v_hi = vf ? e.box_h : e.mid_first + e.mid_count;
    if ((st = check_table(tabs, hd.table_count, e.tab_h, e.ks_h, hd.resize_w, hd.crop_x, cw, h_lo, h_hi, i, "horizontal")) != RART_OK ||
        (st = check_table(tabs, hd.table_count, e.tab_v, e.ks_v, hd.resize_h, hd.crop_y, ch, v_lo, v_hi, i, "vertical")) != RART_OK)
      return st;
  }
  const size_t need_out = (size_t)n * ch * cw * 3;
  if (out_bytes < need_out) {
    rart_set_error("%s: out of %zu bytes required, got %zu", who, need_out, out_bytes);
    return RART_ERR_INVALID;
  }
  const size_t need_ws = (size_t)prefix[n];
  RART_CHECK_ARG(hd.workspace_bytes >= 0 && (size_t)hd.workspace_bytes >= need_ws, "%s: the header's workspace_bytes is below the "
                 "prefix table's total", who);
  if (need_ws > 0 && (!workspace || workspace_bytes < (size_t)hd.workspace_bytes)) {
    rart_set_error("%s: workspace of %zu bytes required, got %zu", who, (size_t)hd.workspace_bytes, workspace_bytes);
    return RART_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* db = (const uint8_t*)plan;
  const rart_resize_desc* ddesc = (const rart_resize_desc*)(db + hd.desc_off);
  if (hd.filter == 0) {
    hipLaunchKernelGGL(k_batch_nearest, dim3(rart_grid_for((size_t)n * ch * cw, kBlock, 256 * 16)), dim3(kBlock), 0, s, ddesc,
                       (const int*)(db + hd.table_off), n, hd.crop_y, hd.crop_x, ch, cw, out);
    RART_CHECK_LAUNCH("rart_resize_batch_u8 (nearest)");
    return RART_OK;
  }
  const long long* dprefix = (const long long*)(db + hd.prefix_off);
  const int* dtabs = (const int*)(db + hd.table_off);
  hipLaunchKernelGGL(k_batch_pass1, dim3(rart_grid_for(need_ws, kBlock, 256 * 16)), dim3(kBlock), 0, s, ddesc, dprefix, dtabs, n,
                     hd.crop_y, hd.crop_x, cw, (uint8_t*)workspace);
  RART_CHECK_LAUNCH("rart_resize_batch_u8 (first pass)");
  hipLaunchKernelGGL(k_batch_pass2, dim3(rart_grid_for(need_out, kBlock, 256 * 16)), dim3(kBlock), 0, s, ddesc, dprefix, dtabs, n,
                     hd.crop_y, hd.crop_x, ch, cw, (const uint8_t*)workspace, out);
  RART_CHECK_LAUNCH("rart_resize_batch_u8 (second pass)");
  return RART_OK;
}

}  // extern "C"
