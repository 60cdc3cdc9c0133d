// OpenCV's resize tables (opencv/modules/imgproc/src/resize.cpp, 4.x) and the rule by which cv2.resize chooses its code, shared by the
// single-size (resize_cv.hip) and the batched variable-size (resize_cv_batch.hip) resize: built on the host in the same float /
// double arithmetic as OpenCV, cached for the process lifetime.
#pragma once
#include "rart_common.h"
#include <math.h>
#include <float.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

namespace rart_cv {
enum { CV_NEAREST = 0, CV_LINEAR = 1, CV_CUBIC = 2, CV_AREA = 3, CV_LANCZOS4 = 4 };
// the code cv2.resize runs (the values of RART_CV_PATH_* in robustart_hip.h)
enum { PATH_NEAREST = 0, PATH_TWO_PASS = 1, PATH_AREA_FLOAT = 2, PATH_AREA_INT = 3 };

inline short sat_short(float v) {
  int i = (int)lrintf(v);                                          // round half to even (default rounding mode)
  return (short)(i < -32768 ? -32768 : (i > 32767 ? 32767 : i));
}
inline void interpolate_cubic(float x, float* c) {
  const float A = -0.75f;
  c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
  c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
  c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
  c[3] = 1.f - c[0] - c[1] - c[2];
}
inline void interpolate_lanczos4(float x, float* c) {
  static const double s45 = 0.70710678118654752440084436210485;
  static const double cs[][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
  if (x < FLT_EPSILON) {
    for (int i = 0; i < 8; ++i) c[i] = 0;
    c[3] = 1;
    return;
  }
  float sum = 0;
  const double y0 = -(x + 3) * M_PI * 0.25, s0 = sin(y0), c0 = cos(y0);
  for (int i = 0; i < 8; ++i) {
    const double y = -(x + 3 - i) * M_PI * 0.25;
    c[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
    sum += c[i];
  }
  sum = 1.f / sum;
  for (int i = 0; i < 8; ++i) c[i] *= sum;
}

// per output index: [first tap source index (may be outside: taps clamp), k0 .. k_{ksize-1}] as int32
struct AxisTable {
  int ksize;
  std::vector<int> data;
};
inline const AxisTable& linear_family_table(int ssize, int dsize, int interp, bool is_x) {
  // cached for the process lifetime: the asynchronous upload reads the host vector after this call returns
  static std::map<std::tuple<int, int, int, bool>, AxisTable> cache;
  std::lock_guard<std::mutex> lk(rart_host_table_mutex());      // (loader threads: see rart_common.h)
  const auto key = std::make_tuple(ssize, dsize, interp, is_x);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  const double inv_scale = (double)dsize / ssize, scale = 1.0 / inv_scale;
  const bool area_mode = interp == CV_AREA;
  const int ksize = interp == CV_CUBIC ? 4 : (interp == CV_LANCZOS4 ? 8 : 2), ksize2 = ksize / 2;
  AxisTable t;
  t.ksize = ksize;
  t.data.assign((size_t)dsize * (ksize + 1), 0);
  for (int d = 0; d < dsize; ++d) {
    float f;
    int s;
    if (!area_mode) {
      f = (float)((d + 0.5) * scale - 0.5);
      s = (int)floorf(f);
      f -= s;
    } else {
      s = (int)floor(d * scale);
      f = (float)((d + 1) - (s + 1) * inv_scale);
      f = f <= 0 ? 0.f : f - floorf(f);
    }
    if (is_x && ksize == 2) {            // the x table pins border samples (resize.cpp: xmin / xmax handling)
      if (s < 0) { f = 0; s = 0; }
      if (s >= ssize - 1) { f = 0; s = ssize - 1; }
    }
    float cbuf[8];
    if (interp == CV_CUBIC) interpolate_cubic(f, cbuf);
    else if (interp == CV_LANCZOS4) interpolate_lanczos4(f, cbuf);
    else { cbuf[0] = 1.f - f; cbuf[1] = f; }
    int* row = &t.data[(size_t)d * (ksize + 1)];
    row[0] = s - (ksize2 - 1);
    for (int k = 0; k < ksize; ++k) row[1 + k] = sat_short(cbuf[k] * 2048.f);
  }
  return cache.emplace(key, std::move(t)).first->second;
}

// AREA (fractional decimation): per output index [count, (source index, alpha as float bits) x max_count]
struct AreaTable {
  int max_count;
  std::vector<int> data;
};
inline const AreaTable& area_table(int ssize, int dsize) {
  static std::map<std::pair<int, int>, AreaTable> cache;
  std::lock_guard<std::mutex> lk(rart_host_table_mutex());      // (loader threads: see rart_common.h)
  const auto key = std::make_pair(ssize, dsize);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  const double scale = (double)ssize / dsize;
  std::vector<std::vector<std::pair<int, float>>> rows(dsize);
  int mx = 0;
  for (int dx = 0; dx < dsize; ++dx) {
    const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
    const double cell = std::min(scale, ssize - fsx1);
    int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
    sx2 = std::min(sx2, ssize - 1);
    sx1 = std::min(sx1, sx2);
    if (sx1 - fsx1 > 1e-3) rows[dx].push_back({sx1 - 1, (float)((sx1 - fsx1) / cell)});
    for (int sx = sx1; sx < sx2; ++sx) rows[dx].push_back({sx, (float)(1.0 / cell)});
    if (fsx2 - sx2 > 1e-3) rows[dx].push_back({sx2, (float)(std::min(std::min(fsx2 - sx2, 1.), cell) / cell)});
    mx = std::max(mx, (int)rows[dx].size());
  }
  AreaTable t;
  t.max_count = mx;
  t.data.assign((size_t)dsize * (1 + 2 * mx), 0);
  for (int dx = 0; dx < dsize; ++dx) {
    int* r = &t.data[(size_t)dx * (1 + 2 * mx)];
    r[0] = (int)rows[dx].size();
    for (size_t k = 0; k < rows[dx].size(); ++k) {
      r[1 + 2 * k] = rows[dx][k].first;
      float a = rows[dx][k].second;
      memcpy(&r[2 + 2 * k], &a, 4);
    }
  }
  return cache.emplace(key, std::move(t)).first->second;
}

// cv2.resize's choice for an h x w source and an rh x rw target.  `interp` becomes the interpolation the chosen code runs with (LINEAR
// with an exact 2 x 2 decimation is executed as AREA); isx / isy are the rounded scales, the cell of PATH_AREA_INT.
inline int choose_path(int h, int w, int rh, int rw, int* interp, int* isx, int* isy) {
  const double scale_x = 1.0 / ((double)rw / w), scale_y = 1.0 / ((double)rh / h);
  *isx = (int)lrint(scale_x), *isy = (int)lrint(scale_y);
  if (*interp == CV_NEAREST) return PATH_NEAREST;
  const bool area_fast = fabs(scale_x - *isx) < DBL_EPSILON && fabs(scale_y - *isy) < DBL_EPSILON;
  if (*interp == CV_LINEAR && area_fast && *isx == 2 && *isy == 2) *interp = CV_AREA;
  if (*interp == CV_AREA && scale_x >= 1 && scale_y >= 1) return area_fast ? PATH_AREA_INT : PATH_AREA_FLOAT;
  return PATH_TWO_PASS;
}
}  // namespace rart_cv
