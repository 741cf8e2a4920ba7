// Device math for the shading kernels: float3 helpers with glam Vec3A semantics and the transcendental
// functions as fixed sequences of IEEE-754 double operations.
//
// Why not __sinf/ocml: the parity contract of this build is bit-for-bit equality of the rendered image
// with the CPU oracle. IEEE +,-,*,/ and sqrt are correctly rounded on both sides (hipcc expands f32/f64
// division and sqrt to the correctly rounded sequences by default), so any function built only from those
// — in one fixed order, compiled with -ffp-contract=off — yields identical bits on gfx950 and x86-64.
// The kernels below follow the classic msun argument reductions and minimax/Taylor polynomials; after the
// final rounding to f32 they are within 1 ulp, the same contract as the f32::sin/cos/acos/exp/ln/powf the
// reference calls (brdf.rs:101-102, :270; light.rs:28-34; common.rs:128-135; openpbr.rs:598, :802).
// That bound is measured, against float64 libm and 120-bit mpmath, by tests/test_math_host.py (DESIGN.md §2 has the
// maxima) on these domains: sincos |x| <= 2^20*pi/2 (see sincos_det), acos [-1, 1], atan2 every pair (tests/test_environment.py), exp [-103.98, 88.73], log every
// finite positive f32, pow every pair with a finite normal result. tests/test_gpu_math.py pins the device bits.
// CDNA4 runs f64 FMA/ADD/MUL at half the f32 vector rate, so a sincos costs ~20 DP ops: cheap next to
// the BVH traversal that dominates a path vertex.
#pragma once

#include <hip/hip_runtime.h>

namespace crt {
namespace dev {

#define CRT_PI 3.14159265358979323846264338327950288f
#define CRT_INF (__builtin_inff())

struct V3 { float x, y, z; };

__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 splat(float s) { return V3{s, s, s}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ V3 operator/(V3 a, V3 b) { return {a.x / b.x, a.y / b.y, a.z / b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float len2(V3 a) { return dot(a, a); }
__device__ __forceinline__ float length(V3 a) { return sqrtf(dot(a, a)); }
__device__ __forceinline__ V3 normalize(V3 a) { return a / sqrtf(dot(a, a)); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y};
}
// f32::max / f32::min / f32::clamp (Rust): the non-NaN operand; the second operand on ties.
__device__ __forceinline__ float rmax(float a, float b) { return (a > b || b != b) ? a : b; }
__device__ __forceinline__ float rmin(float a, float b) { return (a < b || b != b) ? a : b; }
__device__ __forceinline__ float rclamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ float fabs_(float x) { return __uint_as_float(__float_as_uint(x) & 0x7fffffffu); }
// glam Vec3A::min/max/clamp: SSE minps/maxps (second operand on ties or NaN).
__device__ __forceinline__ float smin(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float smax(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ V3 vmin(V3 a, V3 b) { return {smin(a.x, b.x), smin(a.y, b.y), smin(a.z, b.z)}; }
__device__ __forceinline__ V3 vmax(V3 a, V3 b) { return {smax(a.x, b.x), smax(a.y, b.y), smax(a.z, b.z)}; }
__device__ __forceinline__ V3 vclamp(V3 a, V3 lo, V3 hi) { return vmin(vmax(a, lo), hi); }
__device__ __forceinline__ V3 lerp(V3 a, V3 b, float s) { return a * (1.0f - s) + b * s; }  // glam lerp
__device__ __forceinline__ float max_elem(V3 a) { return smax(smax(a.x, a.y), a.z); }
__device__ __forceinline__ float comp(V3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }

// ---- sin / cos ----
// (__host__ too: the environment map's row weights are built on the host from this very sincos_det, environment.cpp)
__host__ __device__ __forceinline__ double ksin(double x) {
  const double S1 = -0.166666666416265235595, S2 = 0.0083333293858894631756, S3 = -0.000198393348360966317347,
               S4 = 0.0000027183114939898219064;
  const double z = x * x;
  const double w = z * z;
  const double r = S3 + z * S4;
  const double s = z * x;
  return (x + s * (S1 + z * S2)) + s * w * r;
}
__host__ __device__ __forceinline__ double kcos(double x) {
  const double C0 = -0.499999997251031003120, C1 = 0.0416666233237390631894, C2 = -0.00138867637746099294692,
               C3 = 0.0000243904487962774090654;
  const double z = x * x;
  const double w = z * z;
  const double r = C2 + z * C3;
  return ((1.0 + z * C0) + w * C1) + (w * z) * r;
}
// Accuracy domain: |x| <= 2^20 * pi/2 (~1.647e6). PIO2_HI has 33 significant bits, so fn * PIO2_HI is exact only
// while fn < 2^20; beyond that the reduction loses bits (cos is 4096 ulp off by 1e7) and the result, though still
// the same bits on host and device, carries no accuracy claim and may leave [-1, 1].
// Out-of-domain rule: NaN gives (NaN, NaN); |x| >= 2^62, +-inf included, gives (sin, cos) = (0, 1) — an f32 that
// large is a multiple of 2^39, its phase is not information. The guard also keeps the double -> integer conversion
// of fn in range: out of range it is undefined in C, x86 and gfx950 answer differently (INT64_MIN vs saturation),
// and an authored thin_film_thickness reaches it (thin_film_lambda). Bits for |x| < 2^62 are those of the unguarded form.
__host__ __device__ __forceinline__ void sincos_det(float xf, float &s, float &c) {
  const double INV_PIO2 = 6.36619772367581382433e-01;
  const double PIO2_HI = 1.57079632673412561417e+00;
  const double PIO2_LO = 6.07710050650619224932e-11;
  const double x = (double)xf;
  if (x != x) { s = xf; c = xf; return; }
  if (!((x < 0.0 ? -x : x) < 4611686018427387904.0)) { s = 0.0f; c = 1.0f; return; }
  const double fn = rint(x * INV_PIO2);
  const double y = (x - fn * PIO2_HI) - fn * PIO2_LO;
  const int n = (int)(long long)fn;
  const double sy = ksin(y), cy = kcos(y);
  switch (n & 3) {
    case 0: s = (float)sy; c = (float)cy; break;
    case 1: s = (float)cy; c = (float)(-sy); break;
    case 2: s = (float)(-sy); c = (float)(-cy); break;
    default: s = (float)(-cy); c = (float)sy; break;
  }
}
__device__ __forceinline__ float cos_det(float x) { float s, c; sincos_det(x, s, c); return c; }

// ---- acos ----
__device__ __forceinline__ double asin_r(double z) {
  const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
               pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
               qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
               qS4 = 7.70381505559019352791e-02;
  const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
  const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
  return p / q;
}
__device__ __forceinline__ float acos_det(float xf) {
  const double PIO2 = 1.57079632679489655800e+00, PI_D = 3.14159265358979311600e+00;
  const double x = (double)xf;
  if (x != x) return xf;
  if (x >= 1.0) return 0.0f;
  if (x <= -1.0) return (float)PI_D;
  const double ax = x < 0.0 ? -x : x;
  if (ax < 0.5) {
    const double z = x * x;
    return (float)(PIO2 - (x + x * asin_r(z)));
  }
  const double z = (1.0 - ax) * 0.5;
  const double s = sqrt(z);
  const double t = 2.0 * (s + s * asin_r(z));
  return (float)(x < 0.0 ? PI_D - t : t);
}

// ---- atan2 ----
// msun's s_atan.c on |y / x| in double: the four-interval reduction (breakpoints 7/16, 11/16, 19/16, 39/16 around
// atan(0.5), atan(1), atan(1.5), atan(inf)) and the degree-11 odd polynomial in its even/odd split.
__device__ __forceinline__ double atan_pos_d(double x) {  // x >= 0, finite
  const double HI0 = 4.63647609000806093515e-01, HI1 = 7.85398163397448278999e-01, HI2 = 9.82793723247329054082e-01,
               HI3 = 1.57079632679489655800e+00;
  const double LO0 = 2.26987774529616870924e-17, LO1 = 3.06161699786838301793e-17, LO2 = 1.39033110312309984516e-17,
               LO3 = 6.12323399573676603587e-17;
  const double T0 = 3.33333333333329318027e-01, T1 = -1.99999999998764832476e-01, T2 = 1.42857142725034663711e-01,
               T3 = -1.11111104054623557880e-01, T4 = 9.09088713343650656196e-02, T5 = -7.69187620504482999495e-02,
               T6 = 6.66107313738753120669e-02, T7 = -5.83357013379057348645e-02, T8 = 4.97687799461593236017e-02,
               T9 = -3.65315727442169155270e-02, T10 = 1.62858201153657823623e-02;
  if (x >= 73786976294838206464.0) return HI3 + LO3;  // 2^66
  double hi = 0.0, lo = 0.0;
  bool reduced = true;
  if (x < 0.4375) reduced = false;
  else if (x < 0.6875) { hi = HI0; lo = LO0; x = (2.0 * x - 1.0) / (2.0 + x); }
  else if (x < 1.1875) { hi = HI1; lo = LO1; x = (x - 1.0) / (x + 1.0); }
  else if (x < 2.4375) { hi = HI2; lo = LO2; x = (x - 1.5) / (1.0 + 1.5 * x); }
  else { hi = HI3; lo = LO3; x = -1.0 / x; }
  const double z = x * x;
  const double w = z * z;
  const double s1 = z * (T0 + w * (T2 + w * (T4 + w * (T6 + w * (T8 + w * T10)))));
  const double s2 = w * (T1 + w * (T3 + w * (T5 + w * (T7 + w * T9))));
  if (!reduced) return x - x * (s1 + s2);
  return hi - ((x * (s1 + s2) - lo) - x);
}
// f32::atan2(y, x) (environment.rs:158) with e_atan2.c's quadrant logic; every case is decided on the operands, the
// double quotient |y / x| of two finite non-zero f32 neither overflows nor underflows. Special cases, in this order:
//   a NaN operand                -> NaN
//   y = +-0:  x > 0 or x = +0    -> +-0 (y itself);   x < 0 or x = -0 -> +-pi      (the u seam of the lat-long map)
//   x = +-0 (y != 0)             -> +-pi/2
//   x = +inf: y = +-inf -> +-pi/4, y finite -> +-0;   x = -inf: y = +-inf -> +-3pi/4, y finite -> +-pi
//   y = +-inf (x finite)         -> +-pi/2
// The sign is y's. pi is (float)PI_D, the f32 ABOVE pi, as f32::atan2 answers; a result below the smallest subnormal
// rounds to a signed zero.
__device__ __forceinline__ float atan2_det(float yf, float xf) {
  const double PI_D = 3.14159265358979311600e+00, PI_LO = 1.2246467991473531772e-16, PIO2 = 1.57079632679489655800e+00;
  const double PIO4 = 7.85398163397448278999e-01, PI3O4 = 2.35619449019234483700e+00;
  if (yf != yf || xf != xf) return __uint_as_float(0x7fc00000u);
  const bool yneg = (__float_as_uint(yf) >> 31) != 0, xneg = (__float_as_uint(xf) >> 31) != 0;
  const double y = (double)fabs_(yf), x = (double)fabs_(xf);
  const double inf = (double)CRT_INF;
  double r;
  if (y == 0.0) { if (!xneg) return yf; r = PI_D; }
  else if (x == 0.0) r = PIO2;
  else if (x == inf) r = y == inf ? (xneg ? PI3O4 : PIO4) : (xneg ? PI_D : 0.0);
  else if (y == inf) r = PIO2;
  else {
    const double z = atan_pos_d(y / x);
    r = xneg ? PI_D - (z - PI_LO) : z;
  }
  return (float)(yneg ? -r : r);
}

// ---- exp / log / pow ----
__device__ __forceinline__ double exp_d(double x) {
  const double INV_LN2 = 1.44269504088896338700e+00;
  const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
  if (x != x) return x;
  if (x > 709.0) return (double)CRT_INF;
  if (x < -745.0) return 0.0;
  const double fk = rint(x * INV_LN2);
  const double r = (x - fk * LN2_HI) - fk * LN2_LO;
  double p = 1.0 / 39916800.0;
  p = 1.0 / 3628800.0 + r * p;
  p = 1.0 / 362880.0 + r * p;
  p = 1.0 / 40320.0 + r * p;
  p = 1.0 / 5040.0 + r * p;
  p = 1.0 / 720.0 + r * p;
  p = 1.0 / 120.0 + r * p;
  p = 1.0 / 24.0 + r * p;
  p = 1.0 / 6.0 + r * p;
  p = 0.5 + r * p;
  p = 1.0 + r * p;
  p = 1.0 + r * p;
  const long long k = (long long)fk;
  const long long k1 = k / 2, k2 = k - k1;
  const double s1 = __longlong_as_double((long long)((unsigned long long)(k1 + 1023) << 52));
  const double s2 = __longlong_as_double((long long)((unsigned long long)(k2 + 1023) << 52));
  return (p * s1) * s2;
}
__device__ __forceinline__ double log_d(double x) {
  const double LN2 = 6.93147180559945286227e-01, SQRT2 = 1.41421356237309514547e+00;
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  long long e = (long long)((b >> 52) & 0x7ff) - 1023;
  double m = __longlong_as_double((long long)((b & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL));
  if (m > SQRT2) { m = m * 0.5; e += 1; }
  const double s = (m - 1.0) / (m + 1.0);
  const double z = s * s;
  double p = 1.0 / 19.0;
  p = 1.0 / 17.0 + z * p;
  p = 1.0 / 15.0 + z * p;
  p = 1.0 / 13.0 + z * p;
  p = 1.0 / 11.0 + z * p;
  p = 1.0 / 9.0 + z * p;
  p = 1.0 / 7.0 + z * p;
  p = 1.0 / 5.0 + z * p;
  p = 1.0 / 3.0 + z * p;
  p = 1.0 + z * p;
  return (double)e * LN2 + 2.0 * s * p;
}
__device__ __forceinline__ float pow_det(float x, float y) {
  if (y == 0.0f) return 1.0f;
  if (x != x || y != y) return __uint_as_float(0x7fc00000u);
  if (x == 1.0f) return 1.0f;
  if (x == 0.0f) return y > 0.0f ? 0.0f : CRT_INF;
  if (x < 0.0f) return __uint_as_float(0x7fc00000u);
  if (x == CRT_INF) return y > 0.0f ? CRT_INF : 0.0f;
  return (float)exp_d((double)y * log_d((double)x));
}
__device__ __forceinline__ float exp_det(float x) { return (float)exp_d((double)x); }
// ln(0) = -inf, ln(<0) = NaN like f32::ln
__device__ __forceinline__ float log_det(float x) {
  if (x != x) return x;
  if (x == 0.0f) return -CRT_INF;
  if (x < 0.0f) return __uint_as_float(0x7fc00000u);
  if (x == CRT_INF) return x;
  return (float)log_d((double)x);
}
__device__ __forceinline__ float pow2_(float x) { return x * x; }
__device__ __forceinline__ float pow5_(float x) { const float x2 = x * x; const float x4 = x2 * x2; return x4 * x; }
__device__ __forceinline__ float pow6_(float x) { const float x2 = x * x; const float x4 = x2 * x2; return x4 * x2; }

}  // namespace dev
}  // namespace crt
