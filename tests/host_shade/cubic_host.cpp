// The device source of the cubic curve span's intersector (kernels/traverse.hip.h: cubic_span, and rounded_cone under it)
// compiled as host C++ for tests/test_cubic_curves.py, behind the stand-in <hip/hip_runtime.h> of profiles/host_shade;
// the test links the builder's bvh_build.cpp beside it for cubic_flatness_depth, the one function that derives a span's
// depth. traverse.hip.h also holds flush_stats, which names two more HIP functions: the shims below.
#include <hip/hip_runtime.h>

static inline uint32_t __shfl_down(uint32_t v, unsigned, int) { return v; }
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) {
  const unsigned long long old = *p;
  *p += v;
  return old;
}

#include "traverse.hip.h"

extern "C" {
// rows: n x 22 floats, o d cp0 cp1 cp2 cp3 r0 r1 t_min t_max; depth[n]. hit[n]; tn: n x 4 floats, t and the outward
// normal (zero on a miss); any[n]: the any-hit form's answer.
void cubic_span_n(const float *rows, const uint32_t *depth, size_t n, int *hit, float *tn, int *any) {
  for (size_t i = 0; i < n; i++) {
    const float *r = rows + 22 * i;
    float cp[12];
    for (int k = 0; k < 12; k++) cp[k] = r[6 + k];
    float t = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    hit[i] = crt::dev::cubic_span<false>(r[0], r[1], r[2], r[3], r[4], r[5], cp, r[18], r[19], depth[i], r[20], r[21], t, nx, ny, nz) ? 1 : 0;
    tn[4 * i] = hit[i] ? t : 0.0f; tn[4 * i + 1] = hit[i] ? nx : 0.0f; tn[4 * i + 2] = hit[i] ? ny : 0.0f; tn[4 * i + 3] = hit[i] ? nz : 0.0f;
    float a, b, c, d;
    any[i] = crt::dev::cubic_span<true>(r[0], r[1], r[2], r[3], r[4], r[5], cp, r[18], r[19], depth[i], r[20], r[21], a, b, c, d) ? 1 : 0;
  }
}
// cp: n x 12 floats; max_width[n] -> depth[n]
void cubic_flatness_depth_n(const float *cp, const float *max_width, size_t n, uint32_t *depth) {
  for (size_t i = 0; i < n; i++) depth[i] = crt::cubic_flatness_depth(cp + 12 * i, max_width[i]);
}
}
