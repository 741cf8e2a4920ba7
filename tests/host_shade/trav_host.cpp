// The device source of the per-ray setup and the scalar watertight triangle test (kernels/traverse.hip.h: setup_ray,
// tri_scalar) compiled as host C++ for tests/test_edge_rays.py, behind the stand-in <hip/hip_runtime.h> of
// profiles/host_shade. traverse.hip.h also holds flush_stats, which names two more HIP functions: the shims below.
#include <hip/hip_runtime.h>

static inline uint32_t __shfl_down(uint32_t v, unsigned, int) { return v; }
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) {
  const unsigned long long old = *p;
  *p += v;
  return old;
}

#include "traverse.hip.h"

extern "C" {
// out: ix, iy, iz, sx, sy, sz (floats) then kx, ky, kz (as ints, in out_k)
void trav_setup_ray(const float o[3], const float d[3], float out[6], int out_k[3]) {
  crt::dev::RayCtx r;
  r.ox = o[0]; r.oy = o[1]; r.oz = o[2]; r.dx = d[0]; r.dy = d[1]; r.dz = d[2];
  crt::dev::setup_ray(r, true);
  out[0] = r.ix; out[1] = r.iy; out[2] = r.iz; out[3] = r.sx; out[4] = r.sy; out[5] = r.sz;
  out_k[0] = r.kx; out_k[1] = r.ky; out_k[2] = r.kz;
}

// setup_ray + tri_scalar, the kernels' fallback test for one ray and triangle v[9]: 1 hit (tuv filled) / 0
int trav_triangle_intersect(const float o[3], const float d[3], const float v[9], float t_min, float t_max,
                            float tuv[3]) {
  crt::dev::RayCtx r;
  r.ox = o[0]; r.oy = o[1]; r.oz = o[2]; r.dx = d[0]; r.dy = d[1]; r.dz = d[2];
  crt::dev::setup_ray(r, true);
  return crt::dev::tri_scalar(r, v, t_min, t_max, tuv[0], tuv[1], tuv[2]) ? 1 : 0;
}
}
