// Batched variable-size resize, OpenCV family, on gfx950: cv2.resize for 8-bit 3-channel images for n images of different sizes in
// one call, bit-exact with rart_cv_resize_u8 (resize_cv.hip) image by image: box -> cv2.resize -> crop window -> mirror
// (imagenet_s_gen.py:138-146, :222-263 with the 'opencv-*' operators).
// Arithmetic: resize_cv.hip's, statement for statement (int16 coefficients from resize_cv_tables.h, int32 horizontal rows, the two
// vertical fixed-point casts, ordered float for fractional AREA, integer sums for integer AREA).  What differs from the single-size
// entry is that cv2.resize chooses its code from the source size and the target (resize_cv_tables.h, choose_path), so the path
// differs from image to image inside one batch and is a field of the descriptor.
// Shape: resize_batch.hip's --
//   rart_cv_resize_batch_plan (host only) writes header | descriptors | prefix table | tables into one host buffer, which crosses the
//   bus in one copy; rart_cv_resize_batch_u8 validates the host copy, then launches
//   k_cvb_pass1 : one thread per sample of the int32 intermediates of the two-pass images.  Image i has mid_count_i * crop_w * 3 of
//               them (the rows of its box that the crop window's vertical taps read), numbered image by image; a thread finds its
//               image by bisection over the prefix table (the other paths have no samples and are never found).  Skipped when the
//               batch has no two-pass image.
//   k_cvb_pass2 : one thread per output sample; every image has crop_h * crop_w * 3, so the image is a division.  It dispatches on
//               the image's path: vertical pass from the intermediate, nearest gather, integer-area sum or float-area
//               accumulation.  The mirror is the column the thread writes to.
// The box is a hard boundary: edge taps clamp to the box, not to the image; the row stride is the image's width.  Sources are read
// byte by byte (decode_batch_gpu hands out views at offsets that are multiples of 3, not of 4).
// Every index a kernel forms is bounded by a value rart_cv_resize_batch_u8 has checked on the host copy.
#include "rart_common.h"
#include "resize_cv_tables.h"
#include <deque>

#pragma clang fp contract(off)

namespace {
using namespace rart_cv;
constexpr int kBlock = 256;
constexpr int kMaxSide = 65535;
constexpr int kMaxTap = 1 << 20;          // |first tap| of a two-pass table row: first + k cannot overflow
constexpr int kMaxCell = 1 << 23;         // pixels of an integer-area cell: 255 * cell fits the int32 sum

static_assert(sizeof(rart_cv_resize_desc) == 64 && sizeof(rart_cv_resize_plan) == 80, "layout documented in robustart_hip.h");
static_assert(RART_CV_PATH_NEAREST == PATH_NEAREST && RART_CV_PATH_TWO_PASS == PATH_TWO_PASS &&
                  RART_CV_PATH_AREA_FLOAT == PATH_AREA_FLOAT && RART_CV_PATH_AREA_INT == PATH_AREA_INT, "path codes of robustart_hip.h");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// horizontal pass: tmp[mid_count][cw][3] int32 per two-pass image = sum_k S[clamp(first + k)] * a_k
__global__ __launch_bounds__(kBlock) void k_cvb_pass1(const rart_cv_resize_desc* __restrict__ desc, const long long* __restrict__ prefix,
                                                      const int* __restrict__ tabs, int n, int cx, int cw, int* __restrict__ tmp) {
  const long long total = prefix[n];
  const long long step = (long long)gridDim.x * kBlock;
  for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < total; g += step) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (prefix[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const rart_cv_resize_desc& d = desc[lo];
    const int local = (int)(g - prefix[lo]);          // < the image's samples, checked to fit an int
    const int p = local / 3, c = local - p * 3;
    const int yo = p / cw, xo = p - yo * cw;
    const int ks = d.ks_x;
    const int* row = tabs + d.tab_x + (size_t)(cx + xo) * (ks + 1);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(d.src) + ((size_t)(d.box_y + d.mid_first + yo) * d.w + d.box_x) * 3 + c;
    int acc = 0;
    for (int k = 0; k < ks; ++k) acc += (int)src[(size_t)clampi(row[0] + k, 0, d.box_w - 1) * 3] * row[1 + k];
    tmp[g] = acc;
  }
}

__global__ __launch_bounds__(kBlock) void k_cvb_pass2(const rart_cv_resize_desc* __restrict__ desc, const long long* __restrict__ prefix,
                                                      const int* __restrict__ tabs, int n, int cy, int cx, int ch, int cw,
                                                      const int* __restrict__ tmp, uint8_t* __restrict__ out) {
  const int row3 = cw * 3;
  const long long total = (long long)n * ch * row3;
  const long long step = (long long)gridDim.x * kBlock;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += step) {
    const long long p = i / row3;
    const int col = (int)(i - p * row3);
    const int img = (int)(p / ch), yo = (int)(p - (long long)img * ch);
    const rart_cv_resize_desc& d = desc[img];
    const int xo = col / 3, c = col - xo * 3;
    const uint8_t* box = reinterpret_cast<const uint8_t*>(d.src) + ((size_t)d.box_y * d.w + d.box_x) * 3 + c;
    const size_t stride = (size_t)d.w * 3;
    int v;
    if (d.path == PATH_TWO_PASS) {                    // vertical pass from the intermediate
      const int ks = d.ks_y, last = d.box_h - 1;
      const int* row = tabs + d.tab_y + (size_t)(cy + yo) * (ks + 1);
      const int* base = tmp + prefix[img] + col;
      if (ks == 2) {
        const int s0 = base[(size_t)(clampi(row[0], 0, last) - d.mid_first) * row3];
        const int s1 = base[(size_t)(clampi(row[0] + 1, 0, last) - d.mid_first) * row3];
        v = (((row[1] * (s0 >> 4)) >> 16) + ((row[2] * (s1 >> 4)) >> 16) + 2) >> 2;
      } else {
        int acc = 0;
        for (int k = 0; k < ks; ++k) acc += base[(size_t)(clampi(row[0] + k, 0, last) - d.mid_first) * row3] * row[1 + k];
        v = (acc + (1 << 21)) >> 22;
      }
    } else if (d.path == PATH_NEAREST) {              // index tables: inside the box, checked on the host copy
      const int sx = tabs[d.tab_x + cx + xo], sy = tabs[d.tab_y + cy + yo];
      v = box[(size_t)sy * stride + (size_t)sx * 3];
    } else if (d.path == PATH_AREA_INT) {             // ks_x x ks_y cells
      const int isx = d.ks_x, isy = d.ks_y;
      const uint8_t* src = box + (size_t)(cy + yo) * isy * stride + (size_t)(cx + xo) * isx * 3;
      int sum = 0;
      for (int y = 0; y < isy; ++y)
        for (int x = 0; x < isx; ++x) sum += src[(size_t)y * stride + (size_t)x * 3];
      v = (isx == 2 && isy == 2) ? (sum + 2) >> 2 : (int)rintf((float)sum * (1.f / (float)(isx * isy)));
    } else {                                          // PATH_AREA_FLOAT: OpenCV's order (columns of a source row, then rows)
      const int* xr = tabs + d.tab_x + (size_t)(cx + xo) * (1 + 2 * d.ks_x);
      const int* yr = tabs + d.tab_y + (size_t)(cy + yo) * (1 + 2 * d.ks_y);
      float sum = 0.f;
      for (int j = 0; j < yr[0]; ++j) {
        const uint8_t* src = box + (size_t)yr[1 + 2 * j] * stride;
        float buf = 0.f;
        for (int k = 0; k < xr[0]; ++k) buf += (float)src[(size_t)xr[1 + 2 * k] * 3] * __int_as_float(xr[2 + 2 * k]);
        const float beta = __int_as_float(yr[2 + 2 * j]);
        sum = j == 0 ? beta * buf : sum + beta * buf;
      }
      v = (int)rintf(sum);
    }
    const int ox = d.flip ? cw - 1 - xo : xo;
    out[p * row3 + ox * 3 + c] = (uint8_t)clampi(v, 0, 255);
  }
}

// the four regions behind one another, each 16-byte aligned
void layout(rart_cv_resize_plan* p) {
  p->desc_off = (int64_t)rart_align_up(sizeof(rart_cv_resize_plan), 16);
  p->prefix_off = p->desc_off + (int64_t)rart_align_up((size_t)p->n * sizeof(rart_cv_resize_desc), 16);
  p->table_off = p->prefix_off + (int64_t)rart_align_up(((size_t)p->n + 1) * sizeof(long long), 16);
  p->total_bytes = p->table_off + p->table_count * (int64_t)sizeof(int);
}

// the per-call arguments and the caller's fields of one descriptor; `who` names the entry in the message
int check_call(const char* who, int n, int interp, int rh, int rw, int cy, int cx, int ch, int cw) {
  RART_CHECK_ARG(n > 0, "%s: image count must be positive, got %d", who, n);
  RART_CHECK_ARG(interp >= 0 && interp <= 4, "%s: interpolation must be a cv2 constant 0..4 (INTER_NEAREST, LINEAR, CUBIC, AREA, "
                 "LANCZOS4), got %d", who, interp);
  RART_CHECK_ARG(rh > 0 && rw > 0 && rh <= kMaxSide && rw <= kMaxSide, "%s: target size %d x %d out of range", who, rh, rw);
  RART_CHECK_ARG(cy >= 0 && cx >= 0 && ch > 0 && cw > 0 && cy <= rh - ch && cx <= rw - cw,
                 "%s: crop window (%d, %d, %d, %d) outside the resized image %d x %d", who, cy, cx, ch, cw, rh, rw);
  return RART_OK;
}
int check_image(const char* who, int i, const rart_cv_resize_desc& e) {
  RART_CHECK_ARG(e.src != 0, "%s: image %d: null source", who, i);
  RART_CHECK_ARG(e.h > 0 && e.w > 0 && e.h <= kMaxSide && e.w <= kMaxSide, "%s: image %d: size %d x %d out of range", who, i, e.h, e.w);
  RART_CHECK_ARG(e.box_y >= 0 && e.box_x >= 0 && e.box_h > 0 && e.box_w > 0 && e.box_y <= e.h - e.box_h && e.box_x <= e.w - e.box_w,
                 "%s: image %d: box (%d, %d, %d, %d) outside the image %d x %d", who, i, e.box_y, e.box_x, e.box_h, e.box_w, e.h, e.w);
  return RART_OK;
}

const char* const kWho = "rart_cv_resize_batch_u8";
// a table of `rows` rows of `width` int32 must lie in the table region
int check_region(int64_t table_count, int off, int rows, int width, int i, const char* which) {
  RART_CHECK_ARG(off >= 0 && (int64_t)off + (int64_t)rows * width <= table_count,
                 "%s: image %d: %s table offset %d (%d rows of %d) outside the table region of %lld", kWho, i, which, off, rows, width,
                 (long long)table_count);
  return RART_OK;
}
// NEAREST: entries [first, first + count) point inside [0, size)
int check_index(const int* tabs, int64_t table_count, int off, int rows, int first, int count, int size, int i, const char* which) {
  const int st = check_region(table_count, off, rows, 1, i, which);
  if (st != RART_OK) return st;
  for (int r = first; r < first + count; ++r)
    RART_CHECK_ARG(tabs[off + r] >= 0 && tabs[off + r] < size, "%s: image %d: %s table entry %d = %d outside the box's [0, %d)", kWho, i,
                   which, r, tabs[off + r], size);
  return RART_OK;
}
// two-pass: rows [first, first + count) of [first tap, ks coefficients]; the taps, clamped to [0, size) as the kernels clamp them, must
// lie in [lo, hi) (the box for the horizontal table, the intermediate's rows for the vertical one)
int check_taps(const int* tabs, int64_t table_count, int off, int ks, int rows, int first, int count, int size, int lo, int hi, int i,
               const char* which) {
  RART_CHECK_ARG(ks == 2 || ks == 4 || ks == 8, "%s: image %d: %s table of %d taps per row (2, 4 or 8)", kWho, i, which, ks);
  const int st = check_region(table_count, off, rows, ks + 1, i, which);
  if (st != RART_OK) return st;
  for (int r = first; r < first + count; ++r) {
    const int t0 = tabs[off + (size_t)r * (ks + 1)];
    RART_CHECK_ARG(t0 >= -kMaxTap && t0 <= kMaxTap, "%s: image %d: %s table row %d: first tap %d out of range", kWho, i, which, r, t0);
    const int a = std::max(0, std::min(size - 1, t0)), b = std::max(0, std::min(size - 1, t0 + ks - 1));
    RART_CHECK_ARG(a >= lo && b < hi, "%s: image %d: %s table row %d taps [%d, %d] outside [%d, %d)", kWho, i, which, r, a, b, lo, hi);
  }
  return RART_OK;
}
// float AREA: rows [first, first + count) of [count, (index, alpha) x ks]; every index inside [0, size)
int check_area(const int* tabs, int64_t table_count, int off, int ks, int rows, int first, int count, int size, int i, const char* which) {
  RART_CHECK_ARG(ks >= 1 && ks <= kMaxSide + 2, "%s: image %d: %s area table of %d entries per row", kWho, i, which, ks);
  const int st = check_region(table_count, off, rows, 1 + 2 * ks, i, which);
  if (st != RART_OK) return st;
  for (int r = first; r < first + count; ++r) {
    const int* row = tabs + off + (size_t)r * (1 + 2 * ks);
    RART_CHECK_ARG(row[0] >= 0 && row[0] <= ks, "%s: image %d: %s area table row %d holds %d entries of at most %d", kWho, i, which, r,
                   row[0], ks);
    for (int k = 0; k < row[0]; ++k)
      RART_CHECK_ARG(row[1 + 2 * k] >= 0 && row[1 + 2 * k] < size, "%s: image %d: %s area table row %d index %d outside the box's [0, %d)",
                     kWho, i, which, r, row[1 + 2 * k], size);
  }
  return RART_OK;
}
}  // namespace

extern "C" {

int rart_cv_resize_batch_plan(const rart_cv_resize_desc* images_host, int n, int interpolation, int resize_h, int resize_w, int crop_y,
                              int crop_x, int crop_h, int crop_w, void* plan_host, size_t capacity, rart_cv_resize_plan* sizes) {
  static const char* who = "rart_cv_resize_batch_plan";
  int st = check_call(who, n, interpolation, resize_h, resize_w, crop_y, crop_x, crop_h, crop_w);
  if (st != RART_OK) return st;
  RART_CHECK_ARG(images_host && (plan_host || sizes), "%s: bad arguments", who);
  RART_CHECK_ARG(((uintptr_t)plan_host & 15) == 0, "%s: plan_host must be 16-byte aligned", who);
  for (int i = 0; i < n; ++i)
    if ((st = check_image(who, i, images_host[i])) != RART_OK) return st;
  rart_cv_resize_plan hd{};
  hd.n = n, hd.interpolation = interpolation, hd.resize_h = resize_h, hd.resize_w = resize_w;
  hd.crop_y = crop_y, hd.crop_x = crop_x, hd.crop_h = crop_h, hd.crop_w = crop_w;
  // the distinct tables of the call: (path, effective interpolation, axis, source size, target size) -> element of the table region.
  // Only the two-taps-per-row tables differ between the axes (the x table pins its border samples).
  std::map<std::tuple<int, int, bool, int, int>, int> used;
  std::vector<const std::vector<int>*> order;
  std::deque<std::vector<int>> nearest;      // NEAREST: built per call (target-size ints each), not cached
  auto place = [&](const std::tuple<int, int, bool, int, int>& key, const std::vector<int>* data) {
    const int off = (int)hd.table_count;
    hd.table_count += (int64_t)data->size();
    order.push_back(data);
    used[key] = off;
    return off;
  };
  auto nearest_table = [&](int ssize, int dsize) {
    const auto key = std::make_tuple((int)PATH_NEAREST, 0, false, ssize, dsize);
    auto it = used.find(key);
    if (it != used.end()) return it->second;
    // k_cv_nearest: x = floor(dx * scale), x = min(x, w - 1), with scale = 1 / (dsize / ssize) in double
    const double scale = 1.0 / ((double)dsize / ssize);
    std::vector<int> t((size_t)dsize);
    for (int d = 0; d < dsize; ++d) {
      const int s = (int)floor(d * scale);
      t[d] = s < ssize - 1 ? s : ssize - 1;
    }
    nearest.push_back(std::move(t));
    return place(key, &nearest.back());
  };
  auto family_table = [&](int ssize, int dsize, int interp, bool is_x, int* ks) {
    const AxisTable& t = linear_family_table(ssize, dsize, interp, is_x);
    *ks = t.ksize;
    const auto key = std::make_tuple((int)PATH_TWO_PASS, interp, is_x && t.ksize == 2, ssize, dsize);
    auto it = used.find(key);
    return it != used.end() ? it->second : place(key, &t.data);
  };
  auto float_area_table = [&](int ssize, int dsize, int* ks) {
    const AreaTable& t = area_table(ssize, dsize);
    *ks = t.max_count;
    const auto key = std::make_tuple((int)PATH_AREA_FLOAT, 0, false, ssize, dsize);
    auto it = used.find(key);
    return it != used.end() ? it->second : place(key, &t.data);
  };
  std::vector<rart_cv_resize_desc> descs(images_host, images_host + n);
  std::vector<long long> prefix((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) {
    rart_cv_resize_desc& d = descs[i];
    d.tab_x = d.ks_x = d.tab_y = d.ks_y = d.mid_first = d.mid_count = 0;
    d.flip = d.flip ? 1 : 0;
    prefix[i + 1] = prefix[i];
    RART_CHECK_ARG(hd.table_count <= 0x3FFFFFFF, "%s: the call's tables exceed 2^30 entries", who);
    int interp = interpolation, isx, isy;
    d.path = choose_path(d.box_h, d.box_w, resize_h, resize_w, &interp, &isx, &isy);
    if (d.path == PATH_NEAREST) {
      d.tab_x = nearest_table(d.box_w, resize_w), d.tab_y = nearest_table(d.box_h, resize_h);
    } else if (d.path == PATH_AREA_INT) {
      RART_CHECK_ARG((long long)isx * isy <= kMaxCell, "%s: image %d: an integer-area cell of %d x %d pixels exceeds 2^23", who, i, isy, isx);
      d.ks_x = isx, d.ks_y = isy;
    } else if (d.path == PATH_AREA_FLOAT) {
      d.tab_x = float_area_table(d.box_w, resize_w, &d.ks_x), d.tab_y = float_area_table(d.box_h, resize_h, &d.ks_y);
    } else {
      d.tab_x = family_table(d.box_w, resize_w, interp, true, &d.ks_x), d.tab_y = family_table(d.box_h, resize_h, interp, false, &d.ks_y);
      // the rows of the box that the vertical pass reads through its (clamped) taps over the crop window: make_plan of resize_cv.hip
      const int* ty = linear_family_table(d.box_h, resize_h, interp, false).data.data();
      int first = d.box_h, last = 0;
      for (int yy = crop_y; yy < crop_y + crop_h; ++yy) {
        const int t0 = ty[(size_t)yy * (d.ks_y + 1)];
        const int a = std::max(0, std::min(d.box_h - 1, t0)), b = std::max(0, std::min(d.box_h - 1, t0 + d.ks_y - 1));
        first = std::min(first, a);
        last = std::max(last, b + 1);
      }
      d.mid_first = first, d.mid_count = last - first;
      const long long items = (long long)d.mid_count * crop_w * 3;
      RART_CHECK_ARG(items <= 0x7FFFFFFF, "%s: image %d: an intermediate of %lld samples exceeds 2^31", who, i, items);
      prefix[i + 1] = prefix[i] + items;
    }
  }
  RART_CHECK_ARG(hd.table_count <= 0x3FFFFFFF, "%s: the call's tables exceed 2^30 entries", who);
  hd.workspace_bytes = (int64_t)rart_align_up((size_t)prefix[n] * sizeof(int), 256);
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
  memcpy(base + hd.desc_off, descs.data(), (size_t)n * sizeof(rart_cv_resize_desc));
  memcpy(base + hd.prefix_off, prefix.data(), ((size_t)n + 1) * sizeof(long long));
  int* tabs = (int*)(base + hd.table_off);
  for (const std::vector<int>* t : order) {
    memcpy(tabs, t->data(), t->size() * sizeof(int));
    tabs += t->size();
  }
  return RART_OK;
}

int rart_cv_resize_batch_u8(const void* plan, const void* plan_host, size_t plan_bytes, void* workspace, size_t workspace_bytes,
                            uint8_t* out, size_t out_bytes, rart_stream_t stream) {
  const char* who = kWho;
  RART_CHECK_ARG(plan && plan_host && out, "%s: bad arguments", who);
  RART_CHECK_ARG(((uintptr_t)plan & 15) == 0 && ((uintptr_t)plan_host & 7) == 0, "%s: the plan must be 16-byte aligned", who);
  RART_CHECK_ARG(plan_bytes >= sizeof(rart_cv_resize_plan), "%s: plan of %zu bytes is shorter than its header", who, plan_bytes);
  const uint8_t* hb = (const uint8_t*)plan_host;
  rart_cv_resize_plan hd;
  memcpy(&hd, hb, sizeof(hd));
  int st = check_call(who, hd.n, hd.interpolation, hd.resize_h, hd.resize_w, hd.crop_y, hd.crop_x, hd.crop_h, hd.crop_w);
  if (st != RART_OK) return st;
  RART_CHECK_ARG(hd.table_count >= 0 && hd.table_count <= 0x3FFFFFFF, "%s: table_count %lld out of range", who, (long long)hd.table_count);
  rart_cv_resize_plan want = hd;
  layout(&want);
  RART_CHECK_ARG(want.desc_off == hd.desc_off && want.prefix_off == hd.prefix_off && want.table_off == hd.table_off &&
                     want.total_bytes == hd.total_bytes, "%s: the header's region offsets do not match its counts", who);
  RART_CHECK_ARG((size_t)hd.total_bytes <= plan_bytes, "%s: the plan holds %lld bytes, plan_bytes says %zu", who,
                 (long long)hd.total_bytes, plan_bytes);
  const rart_cv_resize_desc* d = (const rart_cv_resize_desc*)(hb + hd.desc_off);
  const long long* prefix = (const long long*)(hb + hd.prefix_off);
  const int* tabs = (const int*)(hb + hd.table_off);
  const int n = hd.n, cw = hd.crop_w, ch = hd.crop_h, cx = hd.crop_x, cy = hd.crop_y, rw = hd.resize_w, rh = hd.resize_h;
  RART_CHECK_ARG(prefix[0] == 0, "%s: the prefix table must start at 0", who);
  for (int i = 0; i < n; ++i) {
    const rart_cv_resize_desc& e = d[i];
    if ((st = check_image(who, i, e)) != RART_OK) return st;
    RART_CHECK_ARG(e.path >= PATH_NEAREST && e.path <= PATH_AREA_INT && (e.path == PATH_NEAREST) == (hd.interpolation == CV_NEAREST),
                   "%s: image %d: path code %d out of range for interpolation %d", who, i, e.path, hd.interpolation);
    long long items = 0;
    if (e.path == PATH_TWO_PASS) {
      RART_CHECK_ARG(e.mid_first >= 0 && e.mid_count >= 1 && e.mid_first <= e.box_h - e.mid_count,
                     "%s: image %d: intermediate range [%d, +%d) outside the box's %d rows", who, i, e.mid_first, e.mid_count, e.box_h);
      items = (long long)e.mid_count * cw * 3;
      if ((st = check_taps(tabs, hd.table_count, e.tab_x, e.ks_x, rw, cx, cw, e.box_w, 0, e.box_w, i, "horizontal")) != RART_OK ||
          (st = check_taps(tabs, hd.table_count, e.tab_y, e.ks_y, rh, cy, ch, e.box_h, e.mid_first, e.mid_first + e.mid_count, i,
                           "vertical")) != RART_OK)
        return st;
    } else if (e.path == PATH_NEAREST) {
      if ((st = check_index(tabs, hd.table_count, e.tab_x, rw, cx, cw, e.box_w, i, "column")) != RART_OK ||
          (st = check_index(tabs, hd.table_count, e.tab_y, rh, cy, ch, e.box_h, i, "row")) != RART_OK)
        return st;
    } else if (e.path == PATH_AREA_FLOAT) {
      if ((st = check_area(tabs, hd.table_count, e.tab_x, e.ks_x, rw, cx, cw, e.box_w, i, "column")) != RART_OK ||
          (st = check_area(tabs, hd.table_count, e.tab_y, e.ks_y, rh, cy, ch, e.box_h, i, "row")) != RART_OK)
        return st;
    } else {
      RART_CHECK_ARG(e.ks_x >= 1 && e.ks_y >= 1 && (long long)e.ks_x * e.ks_y <= kMaxCell && (long long)(cx + cw) * e.ks_x <= e.box_w &&
                         (long long)(cy + ch) * e.ks_y <= e.box_h,
                     "%s: image %d: integer-area cells of %d x %d pixels over the crop window reach outside the box %d x %d", who, i, e.ks_y,
                     e.ks_x, e.box_h, e.box_w);
    }
    RART_CHECK_ARG(items <= 0x7FFFFFFF && prefix[i + 1] - prefix[i] == items,
                   "%s: image %d: the prefix table must continue the numbering by the image's %lld intermediate samples", who, i, items);
  }
  const size_t need_out = (size_t)n * ch * cw * 3;
  if (out_bytes < need_out) {
    rart_set_error("%s: out of %zu bytes required, got %zu", who, need_out, out_bytes);
    return RART_ERR_INVALID;
  }
  const size_t need_ws = (size_t)prefix[n] * sizeof(int);
  RART_CHECK_ARG(hd.workspace_bytes >= 0 && (size_t)hd.workspace_bytes >= need_ws, "%s: the header's workspace_bytes is below the "
                 "prefix table's total", who);
  if (need_ws > 0) {
    if (!workspace || workspace_bytes < (size_t)hd.workspace_bytes) {
      rart_set_error("%s: workspace of %zu bytes required, got %zu", who, (size_t)hd.workspace_bytes, workspace_bytes);
      return RART_ERR_WORKSPACE;
    }
    RART_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "%s: the workspace must be 4-byte aligned", who);
  }
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* db = (const uint8_t*)plan;
  const rart_cv_resize_desc* ddesc = (const rart_cv_resize_desc*)(db + hd.desc_off);
  const long long* dprefix = (const long long*)(db + hd.prefix_off);
  const int* dtabs = (const int*)(db + hd.table_off);
  if (need_ws > 0) {
    hipLaunchKernelGGL(k_cvb_pass1, dim3(rart_grid_for((size_t)prefix[n], kBlock, 256 * 16)), dim3(kBlock), 0, s, ddesc, dprefix, dtabs, n,
                       cx, cw, (int*)workspace);
    RART_CHECK_LAUNCH("rart_cv_resize_batch_u8 (horizontal pass)");
  }
  hipLaunchKernelGGL(k_cvb_pass2, dim3(rart_grid_for(need_out, kBlock, 256 * 16)), dim3(kBlock), 0, s, ddesc, dprefix, dtabs, n, cy, cx, ch,
                     cw, (const int*)workspace, out);
  RART_CHECK_LAUNCH("rart_cv_resize_batch_u8 (output pass)");
  return RART_OK;
}

}  // extern "C"
