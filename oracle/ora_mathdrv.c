/* ORACLE — TEST INFRASTRUCTURE ONLY (see ora_math.h header).
 *
 * Batched drivers over ora_math.h and ora_qmc.h, function by function, for tests/test_math_host.py and
 * tests/test_gpu_math.py: the same exports, under the prefixes host_m_ and dev_m_, come from the device source
 * (tests/host_shade/math_host.cpp, math_dev.hip). Arrays in, arrays out; nothing here is product code.
 */
#include <stddef.h>
#include "ora_math.h"
#include "ora_qmc.h"

#define M1(name, TI, TO, expr) \
  void ora_m_##name##_n(const TI *a, size_t n, TO *o) { for (size_t i = 0; i < n; i++) o[i] = (expr); }
#define M2(name, TA, TB, TO, expr) \
  void ora_m_##name##_n(const TA *a, const TB *b, size_t n, TO *o) { for (size_t i = 0; i < n; i++) o[i] = (expr); }

void ora_m_sincos_n(const float *a, size_t n, float *s, float *c) {
  for (size_t i = 0; i < n; i++) ora_sincosf(a[i], &s[i], &c[i]);
}
M1(cos, float, float, ora_cosf(a[i]))
M1(acos, float, float, ora_acosf(a[i]))
M1(exp, float, float, ora_expf(a[i]))
M1(log, float, float, ora_logf(a[i]))
M2(pow, float, float, float, ora_powf(a[i], b[i]))
M2(rmax, float, float, float, ora_max(a[i], b[i]))
M2(rmin, float, float, float, ora_min(a[i], b[i]))
M2(smax, float, float, float, ora_sse_max(a[i], b[i]))
M2(smin, float, float, float, ora_sse_min(a[i], b[i]))
void ora_m_rclamp_n(const float *a, const float *lo, const float *hi, size_t n, float *o) {
  for (size_t i = 0; i < n; i++) o[i] = ora_clamp(a[i], lo[i], hi[i]);
}

M1(pcg_hash, uint32_t, uint32_t, ora_pcg_hash(a[i]))
M2(laine_karras, uint32_t, uint32_t, uint32_t, ora_laine_karras(a[i], b[i]))
M2(owen, uint32_t, uint32_t, uint32_t, ora_owen(a[i], b[i]))
M1(unit_f32, uint32_t, float, ora_u32_to_unit(a[i]))
/* a: n x (x, y, frame, index) */
void ora_m_sampler_new_n(const int32_t *a, size_t n, uint32_t *pattern) {
  for (size_t i = 0; i < n; i++) pattern[i] = ora_sampler_new(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]).pattern;
}
void ora_m_new_domain_n(const uint32_t *pattern, const int32_t *key, size_t n, uint32_t *o) {
  for (size_t i = 0; i < n; i++) {
    OraSampler s = {pattern[i], 0u};
    o[i] = ora_new_domain(s, key[i]).pattern;
  }
}
void ora_m_draw_sample4_n(const uint32_t *pattern, const uint32_t *index, size_t n, float *o) {
  for (size_t i = 0; i < n; i++) {
    OraSampler s = {pattern[i], index[i]};
    ora_draw_sample4(s, o + 4 * i);
  }
}
void ora_m_draw_rnd1_n(const uint32_t *pattern, const uint32_t *index, size_t n, float *o) {
  for (size_t i = 0; i < n; i++) {
    OraSampler s = {pattern[i], index[i]};
    o[i] = ora_draw_rnd1(s);
  }
}
void ora_m_sobol_dirs(uint32_t *o /* 4 * 32 */) {
  for (int d = 0; d < 4; d++)
    for (int b = 0; b < 32; b++) o[32 * d + b] = ORA_SOBOL_DIRS[d][b];
}
/* The oracle draws bit by bit and keeps no sliced table; this is the table the device's layout describes
 * ([(d - 1) * 4 + k][v] = XOR of directions 8k..8k+7 of dimension d picked by the bits of v), from the oracle's
 * own directions. */
void ora_m_sobol_table(uint32_t *o /* 3 * 4 * 256 */) {
  for (int e = 0; e < 3 * 4 * 256; e++) {
    int v = e & 255, k = (e >> 8) & 3, d = (e >> 10) + 1;
    uint32_t x = 0;
    for (int b = 0; b < 8; b++)
      if ((v >> b) & 1) x ^= ORA_SOBOL_DIRS[d][8 * k + b];
    o[e] = x;
  }
}
