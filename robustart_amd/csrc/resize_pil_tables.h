// Pillow's resampling coefficient tables (libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc), shared by the
// single-size (resize_pil.hip) and the batched variable-size (resize_batch.hip) resize: built on the host with the C library's
// sin / cos exactly as Pillow builds them, cached for the process lifetime by (in_size, out_size, filter).
#pragma once
#include "rart_common.h"
#include <math.h>
#include <map>
#include <tuple>
#include <vector>

namespace rart_pil {
inline double sinc_f(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
inline double filter_value(int f, double x) {
  switch (f) {
    case 3: return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;                      // box
    case 1: x = fabs(x); return x < 1.0 ? 1.0 - x : 0.0;                    // bilinear
    case 4: {                                                                // hamming
      x = fabs(x);
      if (x == 0.0) return 1.0;
      if (x >= 1.0) return 0.0;
      x = x * M_PI;
      return sin(x) / x * (0.54 + 0.46 * cos(x));
    }
    case 2: {                                                                // bicubic, a = -0.5
      const double a = -0.5;
      x = fabs(x);
      if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
      if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
      return 0.0;
    }
    case 5: return (x >= -3.0 && x < 3.0) ? sinc_f(x) * sinc_f(x / 3) : 0.0;  // lanczos
  }
  return 0.0;
}
inline double filter_support(int f) {
  switch (f) { case 3: return 0.5; case 1: case 4: return 1.0; case 2: return 2.0; case 5: return 3.0; }
  return 0.0;
}

// table: per output index [xmin, n, k0 .. k_{ksize-1}] as int32
struct CoeffTable {
  int ksize;
  std::vector<int> data;
};
inline const CoeffTable& coeff_table(int in_size, int out_size, int f) {
  static std::map<std::tuple<int, int, int>, CoeffTable> cache;
  std::lock_guard<std::mutex> lk(rart_host_table_mutex());      // (loader threads: see rart_common.h)
  auto key = std::make_tuple(in_size, out_size, f);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = filter_support(f) * fs;
  const int ksize = (int)ceil(support) * 2 + 1;
  CoeffTable t;
  t.ksize = ksize;
  t.data.assign((size_t)out_size * (ksize + 2), 0);
  const double ss = 1.0 / fs;
  std::vector<double> k(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      k[x] = filter_value(f, ((double)(x + xmin) - center + 0.5) * ss);
      ww += k[x];
    }
    int* row = &t.data[(size_t)xx * (ksize + 2)];
    row[0] = xmin;
    row[1] = xmax;
    for (int x = 0; x < xmax; ++x) {
      double v = k[x];
      if (ww != 0.0) v = v / ww;
      row[2 + x] = v < 0 ? (int)(-0.5 + v * 4194304.0) : (int)(0.5 + v * 4194304.0);
    }
  }
  return cache.emplace(key, std::move(t)).first->second;
}
}  // namespace rart_pil
