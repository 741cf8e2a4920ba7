// The device source of the round curve segment's intersector (kernels/traverse.hip.h: rounded_cone) compiled as host C++
// for tests/test_curves.py, behind the stand-in <hip/hip_runtime.h> of profiles/host_shade. traverse.hip.h also holds
// flush_stats, which names two more HIP functions: the shims below.
#include <hip/hip_runtime.h>

static inline uint32_t __shfl_down(uint32_t v, unsigned, int) { return v; }
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) {
  const unsigned long long old = *p;
  *p += v;
  return old;
}

#include "traverse.hip.h"

extern "C" {
// rows: n x 16 floats, o d p0 r0 p1 r1 t_min t_max. hit[n]; tn: n x 4 floats, t and the outward normal (zero on a miss);
// any[n]: the any-hit form's answer.
void curve_rounded_cone_n(const float *rows, size_t n, int *hit, float *tn, int *any) {
  for (size_t i = 0; i < n; i++) {
    const float *r = rows + 16 * i;
    float t = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    hit[i] = crt::dev::rounded_cone<false>(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], r[12], r[13],
                                           r[14], r[15], t, nx, ny, nz) ? 1 : 0;
    tn[4 * i] = hit[i] ? t : 0.0f; tn[4 * i + 1] = hit[i] ? nx : 0.0f; tn[4 * i + 2] = hit[i] ? ny : 0.0f; tn[4 * i + 3] = hit[i] ? nz : 0.0f;
    float a, b, c, d;
    any[i] = crt::dev::rounded_cone<true>(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], r[12], r[13],
                                          r[14], r[15], a, b, c, d) ? 1 : 0;
  }
}
}
