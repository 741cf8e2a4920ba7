// CPU twin of the mapped dome's device functions (tests only): kernels/envmap.hip.h and kernels/dmath.hip.h — the SAME
// source the kernels include — compiled as host C++ behind the HIP stand-in header profiles/host_shade/hip/hip_runtime.h
// and exported over arrays, so tests/test_environment.py can compare them with the numpy restatement (tests/env_ref.py)
// bit for bit, and so that restatement takes its transcendentals from the device source. No vendor atan2f / sinf / acosf
// is on the path. `image` is the byte image crt_environment_tables hands out (host memory).
// Build: tests/env_ref.py (g++ -O1 -ffp-contract=off -shared, as tests/math_drivers.py builds math_host.cpp).
#include <cstddef>
#include <cstdint>

#include "envmap.hip.h"

using namespace crt::dev;

extern "C" {

void host_env_atan2_n(const float *y, const float *x, size_t n, float *o) { for (size_t i = 0; i < n; i++) o[i] = atan2_det(y[i], x[i]); }
void host_env_acos_n(const float *x, size_t n, float *o) { for (size_t i = 0; i < n; i++) o[i] = acos_det(x[i]); }
void host_env_sincos_n(const float *x, size_t n, float *s, float *c) { for (size_t i = 0; i < n; i++) sincos_det(x[i], s[i], c[i]); }

void host_env_direction_to_uv_n(const float *d, size_t n, float *uv) {
  for (size_t i = 0; i < n; i++) env_direction_to_uv(v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), uv[2 * i], uv[2 * i + 1]);
}
void host_env_uv_to_direction_n(const float *uv, size_t n, float *d) {
  for (size_t i = 0; i < n; i++) {
    const V3 r = env_uv_to_direction(uv[2 * i], uv[2 * i + 1]);
    d[3 * i] = r.x; d[3 * i + 1] = r.y; d[3 * i + 2] = r.z;
  }
}
void host_env_bin_n(const float *cdf, uint32_t bins, uint32_t steps, const float *u, size_t n, uint32_t *o) {
  for (size_t i = 0; i < n; i++) o[i] = env_bin(cdf, bins, steps, u[i]);
}
// DomeLight::sample_li with a map: out = direction (3), radiance (3), pdf, some (1.0 / 0.0) per call; zeros for None
void host_env_sample_n(const void *image, const float tint[3], const float *u, const float *v, size_t n, float *out) {
  const EnvHeader *E = static_cast<const EnvHeader *>(image);
  for (size_t i = 0; i < n; i++) {
    V3 dir = splat(0.0f), rad = splat(0.0f);
    float pdf = 0.0f;
    const bool some = env_light_sample(E, v3(tint[0], tint[1], tint[2]), u[i], v[i], dir, rad, pdf);
    float *o = out + 8 * i;
    if (!some) { dir = rad = splat(0.0f); pdf = 0.0f; }
    o[0] = dir.x; o[1] = dir.y; o[2] = dir.z; o[3] = rad.x; o[4] = rad.y; o[5] = rad.z; o[6] = pdf; o[7] = some ? 1.0f : 0.0f;
  }
}
// DomeLight::escaped with a map: out = radiance (3), pdf per call
void host_env_escaped_n(const void *image, const float tint[3], const float *d, size_t n, float *out) {
  const EnvHeader *E = static_cast<const EnvHeader *>(image);
  for (size_t i = 0; i < n; i++) {
    V3 rad;
    float pdf;
    env_light_escaped(E, v3(tint[0], tint[1], tint[2]), v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), rad, pdf);
    float *o = out + 4 * i;
    o[0] = rad.x; o[1] = rad.y; o[2] = rad.z; o[3] = pdf;
  }
}

}  // extern "C"
