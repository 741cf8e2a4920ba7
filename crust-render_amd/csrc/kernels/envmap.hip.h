// Environment-mapped dome lights on the device: the lat-long map's direction <-> texel mapping and its importance
// sampling (environment.rs:39-97 Distribution1D, :156-214 EnvironmentMap) and the mapped arm of DomeLight
// (light.rs:340-388), statement for statement in f32. No vendor atan2f / sinf / acosf anywhere on the path: the
// transcendentals are dmath.hip.h's fixed double sequences, so the same source compiled as host C++
// (tests/host_shade/env_host.cpp) yields the device's bits.
//
// The image (environment.cpp builds it on the host, one allocation, every array on a 256-byte boundary):
//   EnvHeader | texels float4 (r, g, b, conditional func[x]) | rows float2 (conditional integral, marginal func[y]) |
//   conditional CDFs h x (w + 1) | marginal CDF h + 1
// so `escaped` takes radiance and the conditional weight in ONE 16-byte load and the row's two numbers in one 8-byte load.
// A light record names its environment by ID (CrtLight::center[0]); env_lookup turns the id into an image through the
// library's own slot table — a kernel never dereferences a word a caller wrote.
//
// The one departure from the reference: where several CDF entries EQUAL u (zero-weight bins) Rust's binary_search_by
// leaves the choice among them open; env_bin takes the last.
#pragma once

#include "dmath.hip.h"

namespace crt {
namespace dev {

#define CRT_TAU 6.28318530717958647692528676655900577f

struct EnvHeader {  // 256 bytes at the head of the image; offsets are in bytes from the header
  uint32_t w, h;
  float marg_integral;
  uint32_t steps_w, steps_h;  // ceil(log2(n + 1)) of each table length: env_bin's loop count, never derived from a float
  uint32_t off_texels, off_rows, off_ccdf, off_mcdf;
  uint32_t bytes;
  float l2w[9], w2l[9];       // Mat3A columns x, y, z: light_to_world and its inverse
  uint32_t pad[36];
};
static_assert(sizeof(EnvHeader) == 256, "arrays start on 256-byte boundaries");

// The library's table of live environments (environment.cpp): id = generation << 4 | slot; generation 0 names nothing.
constexpr uint32_t kEnvSlots = 16;
struct EnvSlot { const EnvHeader *image; uint32_t generation; uint32_t pad; };
__device__ __forceinline__ const EnvHeader *env_lookup(const EnvSlot *table, uint32_t id) {
  if (!table) return nullptr;
  const EnvSlot s = table[id & (kEnvSlots - 1u)];
  return s.generation == (id >> 4) && (id >> 4) != 0u ? s.image : nullptr;
}

__device__ __forceinline__ const float4 *env_texels(const EnvHeader *E) {
  return reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(E) + E->off_texels);
}
__device__ __forceinline__ const float2 *env_rows(const EnvHeader *E) {
  return reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(E) + E->off_rows);
}
__device__ __forceinline__ const float *env_ccdf(const EnvHeader *E, uint32_t row) {
  return reinterpret_cast<const float *>(reinterpret_cast<const char *>(E) + E->off_ccdf) + (size_t)row * (E->w + 1u);
}
__device__ __forceinline__ const float *env_mcdf(const EnvHeader *E) {
  return reinterpret_cast<const float *>(reinterpret_cast<const char *>(E) + E->off_mcdf);
}
__device__ __forceinline__ V3 mat3_mul(const float m[9], V3 v) {  // glam Mat3A * Vec3A: (x * v.x + y * v.y) + z * v.z
  return (v3(m[0], m[1], m[2]) * v.x + v3(m[3], m[4], m[5]) * v.y) + v3(m[6], m[7], m[8]) * v.z;
}

// f32::rem_euclid(1.0): r = x % 1 (exact), r < 0 -> r + 1, which may round to 1.0 — the caller's min(w - 1) guards it.
__device__ __forceinline__ float rem_euclid1(float x) {
  if (x != x || fabs_(x) == CRT_INF) return __uint_as_float(0x7fc00000u);
  if (!(fabs_(x) < 8388608.0f)) return 0.0f;  // every f32 that large is an integer
  const float r = x - (float)(int)x;          // truncation; exact
  return r < 0.0f ? r + 1.0f : r;
}
// Rust's `(f as usize).min(n - 1)`: the cast saturates and sends NaN to 0. A C conversion of NaN or of an
// out-of-range value is undefined (x86 and gfx950 answer differently), so both are decided before converting.
__device__ __forceinline__ uint32_t env_index(float f, uint32_t n) {
  if (!(f >= 0.0f)) return 0u;
  if (f >= (float)n) return n - 1u;
  return (uint32_t)f;
}

// environment.rs:156-160
__device__ __forceinline__ void env_direction_to_uv(V3 d, float &u, float &v) {
  const float vv = acos_det(rclamp(d.y, -1.0f, 1.0f)) / CRT_PI;
  const float uu = 0.5f + atan2_det(d.x, -d.z) / CRT_TAU;
  u = rem_euclid1(uu);
  v = rclamp(vv, 0.0f, 1.0f);
}
// environment.rs:163-168
__device__ __forceinline__ V3 env_uv_to_direction(float u, float v) {
  const float theta = v * CRT_PI;
  const float phi = (u - 0.5f) * CRT_TAU;
  float st, ct, sp, cp;
  sincos_det(theta, st, ct);
  sincos_det(phi, sp, cp);
  return v3(st * sp, ct, -st * cp);
}
// environment.rs:208-214
__device__ __forceinline__ float env_solid_angle_pdf(float pdf_uv, float v) {
  float st, ct;
  sincos_det(v * CRT_PI, st, ct);
  if (st <= 0.0f) return 0.0f;
  return pdf_uv / (2.0f * CRT_PI * CRT_PI * st);
}
// Distribution1D::pdf (environment.rs:90-96)
__device__ __forceinline__ float env_pdf1(float func, float integral) { return integral > 0.0f ? func / integral : 1.0f; }

// The bin of Distribution1D::sample (environment.rs:72-78): min(the largest i with cdf[i] <= u, n - 1); a NaN u takes
// the last bin and a negative one the first, as the reference's comparator decides them. The answer is the number of
// INTERIOR entries cdf[1 .. n - 1] that are not above u, found by a bisection of a fixed number of steps.
__device__ __forceinline__ uint32_t env_bin(const float *cdf, uint32_t n, uint32_t steps, float u) {
  uint32_t lo = 0, len = n - 1u;
  for (uint32_t s = 0; s < steps; s++) {
    const uint32_t half = len >> 1;
    const uint32_t mid = lo + half;                            // <= n - 1: cdf[1 + mid] is inside the n + 1 entries
    const bool right = len > 0u && !(cdf[1u + mid] > u);
    lo = right ? mid + 1u : lo;
    len = right ? len - half - 1u : half;
  }
  return lo;
}
// Distribution1D::sample (environment.rs:70-87) without its pdf: x in [0, 1] and the bin.
__device__ __forceinline__ float env_sample1(const float *cdf, uint32_t n, uint32_t steps, float u, uint32_t &bin) {
  bin = env_bin(cdf, n, steps, u);
  const float c0 = cdf[bin], c1 = cdf[bin + 1u];
  const float span = c1 - c0;
  const float within = span > 0.0f ? (u - c0) / span : 0.5f;
  return ((float)bin + within) / (float)n;
}

// The texel along one local direction (environment.rs:171-176), with the (u, v) and the row it was found at.
__device__ __forceinline__ float4 env_texel_at(const EnvHeader *E, V3 local, float &v, uint32_t &y) {
  float u;
  env_direction_to_uv(local, u, v);
  const uint32_t x = env_index(u * (float)E->w, E->w);
  y = env_index(v * (float)E->h, E->h);
  return env_texels(E)[(size_t)y * E->w + x];
}
// EnvironmentMap::radiance alone: what `sample` looks up again along the direction it drew.
__device__ __forceinline__ V3 env_radiance(const EnvHeader *E, V3 local) {
  float v;
  uint32_t y;
  const float4 t = env_texel_at(E, local, v, y);
  return v3(t.x, t.y, t.z);
}
// EnvironmentMap::radiance and ::pdf of one local direction (environment.rs:171-176, :194-202): the reference maps the
// direction twice to the same (u, v); here once.
__device__ __forceinline__ void env_lookup_dir(const EnvHeader *E, V3 local, V3 &texel, float &pdf) {
  float v;
  uint32_t y;
  const float4 t = env_texel_at(E, local, v, y);
  texel = v3(t.x, t.y, t.z);
  if (E->marg_integral <= 0.0f) { pdf = 0.0f; return; }
  const float2 row = env_rows(E)[y];
  pdf = env_solid_angle_pdf(env_pdf1(t.w, row.x) * env_pdf1(row.y, E->marg_integral), v);
}
// EnvironmentMap::sample (environment.rs:181-190); u2 inverts the marginal (rows), u1 the row's conditional.
__device__ __forceinline__ bool env_sample(const EnvHeader *E, float u1, float u2, V3 &direction, V3 &texel, float &pdf) {
  if (E->marg_integral <= 0.0f) return false;
  uint32_t row, col;
  const float v = env_sample1(env_mcdf(E), E->h, E->steps_h, u2, row);
  const float2 rw = env_rows(E)[row];
  const float pdf_v = env_pdf1(rw.y, E->marg_integral);
  const float u = env_sample1(env_ccdf(E, row), E->w, E->steps_w, u1, col);
  const float pdf_u = env_pdf1(env_texels(E)[(size_t)row * E->w + col].w, rw.x);
  direction = env_uv_to_direction(u, v);
  pdf = env_solid_angle_pdf(pdf_u * pdf_v, v);
  if (!(pdf > 0.0f)) return false;
  texel = env_radiance(E, direction);  // looked up again, as upstream: at a texel boundary it may be a neighbour
  return true;
}

// DomeLight::escaped with a map (light.rs:340-355, :385-388): every direction is covered.
__device__ __forceinline__ void env_light_escaped(const EnvHeader *E, V3 tint, V3 direction, V3 &radiance, float &pdf) {
  V3 texel;
  env_lookup_dir(E, mat3_mul(E->w2l, direction), texel, pdf);
  radiance = tint * texel;
}
// DomeLight::sample_li with a map (light.rs:358-383)
__device__ __forceinline__ bool env_light_sample(const EnvHeader *E, V3 tint, float u, float v, V3 &direction, V3 &radiance,
                                                 float &pdf) {
  V3 local, texel;
  if (!env_sample(E, u, v, local, texel, pdf)) return false;
  direction = normalize(mat3_mul(E->l2w, local));
  radiance = tint * texel;
  return true;
}

}  // namespace dev
}  // namespace crt
