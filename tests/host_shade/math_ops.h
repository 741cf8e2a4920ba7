// The functions of kernels/dmath.hip.h and kernels/qmc.hip.h as element-wise operations over arrays (tests only), one
// list for both builds of the device source: tests/host_shade/math_host.cpp runs each as a host loop (host_m_*_n),
// tests/host_shade/math_dev.hip as one small kernel each (dev_m_*_n). The exports mirror oracle/ora_mathdrv.c.
// In an expression a[i], b[i], c[i] are the operands of element i.
#pragma once
#include <cstddef>
#include <cstdint>
#include "dmath.hip.h"
#include "qmc.hip.h"

namespace crt_math_test {
using namespace crt::dev;

// OP1(name, in, out, expr)   OP2(name, in a, in b, out, expr)   OP3(name, T, expr): three inputs of T, output T
#define CRT_MATH_OPS(OP1, OP2, OP3)                                                           \
  OP1(cos, float, float, cos_det(a[i]))                                                       \
  OP1(acos, float, float, acos_det(a[i]))                                                     \
  OP1(exp, float, float, exp_det(a[i]))                                                       \
  OP1(log, float, float, log_det(a[i]))                                                       \
  OP2(pow, float, float, float, pow_det(a[i], b[i]))                                          \
  OP2(rmax, float, float, float, rmax(a[i], b[i]))                                            \
  OP2(rmin, float, float, float, rmin(a[i], b[i]))                                            \
  OP2(smax, float, float, float, smax(a[i], b[i]))                                            \
  OP2(smin, float, float, float, smin(a[i], b[i]))                                            \
  OP3(rclamp, float, rclamp(a[i], b[i], c[i]))                                                \
  OP1(pcg_hash, uint32_t, uint32_t, pcg_hash(a[i]))                                           \
  OP2(laine_karras, uint32_t, uint32_t, uint32_t, laine_karras(a[i], b[i]))                   \
  OP2(owen, uint32_t, uint32_t, uint32_t, owen(a[i], b[i]))                                   \
  OP1(unit_f32, uint32_t, float, unit_f32(a[i]))                                              \
  OP2(new_domain, uint32_t, int32_t, uint32_t, new_domain(Sampler{a[i], 0u}, b[i]).pattern)   \
  OP2(draw_rnd1, uint32_t, uint32_t, float, draw_rnd1(Sampler{a[i], b[i]}))                   \
  /* the arithmetic the bit-exact contract stands on: one IEEE operation each */              \
  OP2(add_f32, float, float, float, a[i] + b[i])                                              \
  OP2(sub_f32, float, float, float, a[i] - b[i])                                              \
  OP2(mul_f32, float, float, float, a[i] * b[i])                                              \
  OP2(div_f32, float, float, float, a[i] / b[i])                                              \
  OP1(sqrt_f32, float, float, sqrtf(a[i]))                                                    \
  OP2(add_f64, double, double, double, a[i] + b[i])                                           \
  OP2(sub_f64, double, double, double, a[i] - b[i])                                           \
  OP2(mul_f64, double, double, double, a[i] * b[i])                                           \
  OP2(div_f64, double, double, double, a[i] / b[i])                                           \
  OP1(sqrt_f64, double, double, sqrt(a[i]))                                                   \
  OP1(f32_to_f64, float, double, (double)a[i])                                                \
  OP1(f64_to_f32, double, float, (float)a[i])                                                 \
  OP1(rint_f64, double, double, rint(a[i]))

}  // namespace crt_math_test
