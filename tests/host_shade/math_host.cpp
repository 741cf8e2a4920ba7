// CPU twin of tests/host_shade/math_dev.hip (tests only): kernels/dmath.hip.h and kernels/qmc.hip.h — the SAME source the
// kernels include — compiled as host C++ behind the HIP stand-in header profiles/host_shade/hip/hip_runtime.h and
// exported function by function with the signatures of oracle/ora_mathdrv.c, so tests/test_math_host.py can compare the
// two element by element and judge both against libm / mpmath without a GPU.
// Build: tests/math_drivers.py (g++ -O1 -ffp-contract=off -shared, as tests/test_shading_seam_host.py builds seam_host.cpp).
#include "math_ops.h"

using namespace crt_math_test;

static uint32_t g_tab[kSobolLdsWords];
static bool g_tab_ready = false;
static const uint32_t *sobol_tab() {
  if (!g_tab_ready) { sobol_tables_init(g_tab); g_tab_ready = true; }
  return g_tab;
}

extern "C" {

#define H1(name, TI, TO, expr) \
  void host_m_##name##_n(const TI *a, size_t n, TO *o) { for (size_t i = 0; i < n; i++) o[i] = (expr); }
#define H2(name, TA, TB, TO, expr) \
  void host_m_##name##_n(const TA *a, const TB *b, size_t n, TO *o) { for (size_t i = 0; i < n; i++) o[i] = (expr); }
#define H3(name, T, expr) \
  void host_m_##name##_n(const T *a, const T *b, const T *c, size_t n, T *o) { for (size_t i = 0; i < n; i++) o[i] = (expr); }
CRT_MATH_OPS(H1, H2, H3)

void host_m_sincos_n(const float *a, size_t n, float *s, float *c) {
  for (size_t i = 0; i < n; i++) sincos_det(a[i], s[i], c[i]);
}
void host_m_dot_n(const float *a, const float *b, size_t n, float *o) {  // a, b: n x 3
  for (size_t i = 0; i < n; i++) o[i] = dot(v3(a[3 * i], a[3 * i + 1], a[3 * i + 2]), v3(b[3 * i], b[3 * i + 1], b[3 * i + 2]));
}
void host_m_normalize_n(const float *a, size_t n, float *o) {  // a, o: n x 3
  for (size_t i = 0; i < n; i++) {
    const V3 r = normalize(v3(a[3 * i], a[3 * i + 1], a[3 * i + 2]));
    o[3 * i] = r.x; o[3 * i + 1] = r.y; o[3 * i + 2] = r.z;
  }
}
void host_m_sampler_new_n(const int32_t *a, size_t n, uint32_t *pattern) {  // a: n x (x, y, frame, index)
  for (size_t i = 0; i < n; i++) pattern[i] = sampler_new(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]).pattern;
}
void host_m_draw_sample4_n(const uint32_t *pattern, const uint32_t *index, size_t n, float *o) {  // o: n x 4
  const uint32_t *tab = sobol_tab();
  for (size_t i = 0; i < n; i++) draw_sample4(Sampler{pattern[i], index[i]}, o + 4 * i, tab);
}
void host_m_sobol_dirs(uint32_t *o /* 4 * 32 */) {
  for (int d = 0; d < 4; d++)
    for (int b = 0; b < 32; b++) o[32 * d + b] = kSobolDirs[d][b];
}
void host_m_sobol_table(uint32_t *o /* kSobolLdsWords */) {
  const uint32_t *tab = sobol_tab();
  for (int e = 0; e < kSobolLdsWords; e++) o[e] = tab[e];
}

}  // extern "C"
