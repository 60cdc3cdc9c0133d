// libjpeg's ISLOW integer IDCT (jidctint.c) and the fixed-point constants of its DCT pair, shared by the jpeg_compression
// corruption (corrupt_jpeg.hip) and the JPEG reader's device stage (jpeg_decode.hip).
#pragma once

namespace {
#define F_0_298 2446
#define F_0_390 3196
#define F_0_541 4433
#define F_0_765 6270
#define F_0_899 7373
#define F_1_175 9633
#define F_1_501 12299
#define F_1_847 15137
#define F_1_961 16069
#define F_2_053 16819
#define F_2_562 20995
#define F_3_072 25172

__device__ __forceinline__ int ds(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jidctint.c, one 1-D pass, descale by SH
template <int SH>
__device__ __forceinline__ void idct8(int* x, int s) {
  const int x0 = x[0], x1 = x[s], x2 = x[2 * s], x3 = x[3 * s], x4 = x[4 * s], x5 = x[5 * s], x6 = x[6 * s],
            x7 = x[7 * s];
  int z1 = (x2 + x6) * F_0_541;
  const int t2 = z1 - x6 * F_1_847, t3 = z1 + x2 * F_0_765;
  const int t0 = (x0 + x4) << 13, t1 = (x0 - x4) << 13;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a0 = x7, a1 = x5, a2 = x3, a3 = x1;
  z1 = a0 + a3;
  int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const int z5 = (z3 + z4) * F_1_175;
  a0 *= F_0_298; a1 *= F_2_053; a2 *= F_3_072; a3 *= F_1_501;
  z1 *= -F_0_899; z2 *= -F_2_562;
  z3 = z3 * -F_1_961 + z5;
  z4 = z4 * -F_0_390 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  x[0] = ds(t10 + a3, SH); x[7 * s] = ds(t10 - a3, SH);
  x[s] = ds(t11 + a2, SH); x[6 * s] = ds(t11 - a2, SH);
  x[2 * s] = ds(t12 + a1, SH); x[5 * s] = ds(t12 - a1, SH);
  x[3 * s] = ds(t13 + a0, SH); x[4 * s] = ds(t13 - a0, SH);
}
}  // namespace
