// Volume regions on the device: the reference's DensityField, VolumeRegion, PhaseMix and Volumes (volume.rs:52-536)
// restated operation for operation — one source for the seam kernels (volume_seam.hip) and, behind the HIP stand-in
// header, for the host twin the tests compare with (tests/host_shade/volume_host.cpp). Compile with -ffp-contract=off.
// log / exp are log_det / exp_det (dmath.hip.h), the phase functions medium.rs:148-184 (shade.hip.h).
//
// Departures from the reference, all named in DESIGN.md §2:
//   1. A WALK IS BOUNDED. volume.rs:429 and :517 are `loop {}`: a NaN distance never satisfies `t >= end`, and a ray
//      whose local direction is below 1e-9 on every axis with t_max = inf has end = inf. Both walks here are `for` loops
//      whose trip count IS the bound: after CRT_VOLUME_MAX_STEPS collision candidates they fall out with status
//      CRT_VOLUME_STEP_LIMIT and an all-zero result. A walk of majorant optical depth tau takes Poisson(tau) candidates.
//   2. At most CRT_VOLUME_MAX_REGIONS regions (the reference's Vecs are unbounded): a lane's spans and lobes live in
//      fixed columns. Noise octaves are limited to CRT_VOLUME_MAX_OCTAVES by crt_volumes_new.
//   3. The placement is a 3x4 affine, world_to_local the library's affine_inverse (scene.cpp), not glam's Mat4::inverse.
// Float -> integer casts: Rust saturates and sends NaN to 0 (`base.x as i32`, `i.max(0.0) as usize`); C leaves them
// undefined and gfx950 and x86 disagree, so both cases are decided BEFORE converting (as env_index does). Integer
// wrap-around happens in uint32_t.
// The random stream is the project's own (openqmc::pcg::Rng is not in the reference tree, so parity with it is
// unpinned): u = unit_f32(pcg_hash(s)); s = s * 747796405u + 2891336453u; the first s is the query's seed.
//
// Per-lane state: a lane carries up to eight (a, b) spans and eight lobe weights across a walk. A runtime-indexed
// private array goes to scratch, so they are columns the caller owns — LDS [region][thread] in the kernels (24 KB at 256
// threads), plain arrays in the host twin — addressed as base[r * stride]. Which regions a lane crosses is a bit mask
// in a register. Region records are wave-uniform: the kernels read them through a const __restrict__ kernel argument
// with a uniform index (scalar loads); grid data is read with plain vector loads.
#pragma once

#include "shade.hip.h"

namespace crt {
namespace dev {

constexpr uint32_t kVolMaxRegions = CRT_VOLUME_MAX_REGIONS;
constexpr uint32_t kVolMagic = 0x314c4f56u;  // "VOL1"

struct VolHeader {  // 256 bytes
  uint32_t magic, n_regions, region_bytes, off_regions;
  uint32_t off_grid, grid_floats, bytes, pad[57];
};
static_assert(sizeof(VolHeader) == 256, "volume image header");

// What VolumeRegion::new derives (volume.rs:205-230), as the walk reads it.
struct VolRegionRec {  // 176 bytes
  float w2l[12];                    // affine_inverse(local_to_world): three columns, translation
  float half[3]; float majorant;    // majorant_sigma_t
  float bmin[3]; uint32_t field;    // world AABB of the eight corners | CRT_VOLUME_HOMOGENEOUS / _NOISE / _GRID
  float bmax[3]; float g;           // g clamped to +-0.99
  float sigma_s[3]; float noise_scale;       // coefficients * density_scale
  float sigma_a[3]; float noise_gain;
  float emission[3]; float noise_lacunarity;
  float noise_threshold; uint32_t noise_octaves, noise_seed, grid_off;  // grid_off: first float in the image's grid data
  uint32_t nx, ny, nz, pad;
};
static_assert(sizeof(VolRegionRec) == 176, "volume region record");

__device__ __forceinline__ float vol_next_f32(uint32_t &s) {
  const float u = unit_f32(pcg_hash(s));
  s = s * 747796405u + 2891336453u;
  return u;
}

// `x as i32` (Rust): NaN -> 0, saturating.
__device__ __forceinline__ int32_t vol_f32_as_i32(float x) {
  if (x != x) return 0;
  if (x >= 2147483648.0f) return 2147483647;
  if (x <= -2147483648.0f) return (int32_t)0x80000000u;
  return (int32_t)x;
}
// `x as usize` for x that is never negative here (it is max(i, 0)), clamped to hi as `.min(n - 1)` does: NaN -> 0.
__device__ __forceinline__ uint32_t vol_f32_as_index(float x, uint32_t hi) {
  if (!(x > 0.0f)) return 0u;
  if (x >= 4294967040.0f) return hi;
  const uint32_t i = (uint32_t)x;
  return i < hi ? i : hi;
}

__device__ __forceinline__ float vol_hash3(uint32_t ix, uint32_t iy, uint32_t iz, uint32_t seed) {  // volume.rs:88-99
  uint32_t h = (ix * 0x8da6b343u) ^ (iy * 0xd8163841u) ^ (iz * 0xcb1ab31fu) ^ (seed * 0x9e3779b9u);
  h ^= h >> 15;
  h *= 0x2c1b3c6du;
  h ^= h >> 12;
  h *= 0x297a2d39u;
  h ^= h >> 15;
  return (float)(h >> 8) / 16777216.0f;
}
__device__ __forceinline__ float vol_smoothstep(float t) { return t * t * (3.0f - 2.0f * t); }  // volume.rs:101-103

__device__ __forceinline__ float vol_value_noise(V3 p, float freq, uint32_t seed) {  // volume.rs:106-125
  const V3 q = p * freq;
  const V3 base = v3(floorf(q.x), floorf(q.y), floorf(q.z));
  const uint32_t ix = (uint32_t)vol_f32_as_i32(base.x), iy = (uint32_t)vol_f32_as_i32(base.y), iz = (uint32_t)vol_f32_as_i32(base.z);
  const V3 f = q - base;
  const float fx = vol_smoothstep(f.x), fy = vol_smoothstep(f.y), fz = vol_smoothstep(f.z);
  const float c0 = vol_hash3(ix, iy, iz, seed), c1 = vol_hash3(ix + 1u, iy, iz, seed);
  const float c2 = vol_hash3(ix, iy + 1u, iz, seed), c3 = vol_hash3(ix + 1u, iy + 1u, iz, seed);
  const float c4 = vol_hash3(ix, iy, iz + 1u, seed), c5 = vol_hash3(ix + 1u, iy, iz + 1u, seed);
  const float c6 = vol_hash3(ix, iy + 1u, iz + 1u, seed), c7 = vol_hash3(ix + 1u, iy + 1u, iz + 1u, seed);
  const float x00 = c0 + (c1 - c0) * fx;
  const float x10 = c2 + (c3 - c2) * fx;
  const float x01 = c4 + (c5 - c4) * fx;
  const float x11 = c6 + (c7 - c6) * fx;
  const float y0 = x00 + (x10 - x00) * fy;
  const float y1 = x01 + (x11 - x01) * fy;
  return y0 + (y1 - y0) * fz;
}

__device__ __forceinline__ float vol_fbm(V3 p, float scale, uint32_t octaves, float gain, float lacunarity, uint32_t seed) {  // volume.rs:128-141
  octaves = octaves < 1u ? 1u : octaves;
  float sum = 0.0f, norm = 0.0f, amp = 1.0f, freq = scale;
  for (uint32_t o = 0; o < octaves; o++) {
    sum += amp * vol_value_noise(p, freq, seed + o);
    norm += amp;
    amp *= gain;
    freq *= lacunarity;
  }
  return sum / rmax(norm, 1e-6f);
}

// coord of grid_trilinear (volume.rs:146-156)
__device__ __forceinline__ void vol_grid_coord(float v, uint32_t n, uint32_t &i0, uint32_t &i1, float &f) {
  const float x = v * (float)n - 0.5f;
  const float i = floorf(x);
  const float fr = x - i;
  i0 = vol_f32_as_index(rmax(i, 0.0f), n - 1u);
  i1 = i0 + 1u < n - 1u ? i0 + 1u : n - 1u;
  f = i < 0.0f ? 0.0f : rmin(fr, 1.0f);
}
__device__ __forceinline__ float vol_grid_trilinear(V3 u, uint32_t nx, uint32_t ny, uint32_t nz, const float *data) {  // volume.rs:144-170
  uint32_t x0, x1, y0, y1, z0, z1;
  float fx, fy, fz;
  vol_grid_coord(u.x, nx, x0, x1, fx);
  vol_grid_coord(u.y, ny, y0, y1, fy);
  vol_grid_coord(u.z, nz, z0, z1, fz);
  const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy}, wz[2] = {1.0f - fz, fz};
  const uint32_t xs[2] = {x0, x1}, ys[2] = {y0, y1}, zs[2] = {z0, z1};
  float out = 0.0f;
#pragma unroll
  for (int c = 0; c < 2; c++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int a = 0; a < 2; a++)
        out += wz[c] * wy[b] * wx[a] * data[(size_t)xs[a] + (size_t)nx * ((size_t)ys[b] + (size_t)ny * (size_t)zs[c])];
  return out;
}

// DensityField::density (volume.rs:52-71) at u in local [0, 1]^3
__device__ __forceinline__ float vol_field_density(const VolRegionRec &R, const float *grid, V3 u) {
  if (R.field == CRT_VOLUME_NOISE) {
    const float fbm = vol_fbm(u, R.noise_scale, R.noise_octaves, R.noise_gain, R.noise_lacunarity, R.noise_seed);
    const float t = rclamp(R.noise_threshold, 0.0f, 0.999f);
    return rmax((fbm - t) / (1.0f - t), 0.0f);
  }
  if (R.field == CRT_VOLUME_GRID) return vol_grid_trilinear(u, R.nx, R.ny, R.nz, grid + R.grid_off);
  return 1.0f;
}

__device__ __forceinline__ V3 vol_w2l_vector(const VolRegionRec &R, V3 p) {  // transform_vector3
  V3 res = v3(R.w2l[0], R.w2l[1], R.w2l[2]) * p.x;
  res = res + v3(R.w2l[3], R.w2l[4], R.w2l[5]) * p.y;
  res = res + v3(R.w2l[6], R.w2l[7], R.w2l[8]) * p.z;
  return res;
}
__device__ __forceinline__ V3 vol_w2l_point(const VolRegionRec &R, V3 p) {  // transform_point3
  return vol_w2l_vector(R, p) + v3(R.w2l[9], R.w2l[10], R.w2l[11]);
}

// VolumeRegion::density (volume.rs:234-242)
__device__ __forceinline__ float vol_region_density(const VolRegionRec &R, const float *grid, V3 p_world) {
  const V3 p = vol_w2l_point(R, p_world);
  const V3 h = v3(R.half[0], R.half[1], R.half[2]);
  if (fabs_(p.x) > h.x || fabs_(p.y) > h.y || fabs_(p.z) > h.z) return 0.0f;
  const V3 u = (p + h) / (h * 2.0f);
  return vol_field_density(R, grid, u);
}

// VolumeRegion::intersect (volume.rs:248-274): the local direction is NOT renormalised
__device__ __forceinline__ bool vol_region_intersect(const VolRegionRec &R, V3 ro, V3 rd, float &t0, float &t1) {
  const V3 o = vol_w2l_point(R, ro);
  const V3 d = vol_w2l_vector(R, rd);
  t0 = 0.0f;
  t1 = CRT_INF;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float h = R.half[a], da = comp(d, a), oa = comp(o, a);
    if (fabs_(da) < 1e-9f) {
      if (fabs_(oa) > h) return false;
      continue;
    }
    const float inv = 1.0f / da;
    float ta = (-h - oa) * inv;
    float tb = (h - oa) * inv;
    if (ta > tb) { const float s = ta; ta = tb; tb = s; }
    t0 = rmax(t0, ta);
    t1 = rmin(t1, tb);
    if (t1 <= t0) return false;
  }
  return true;
}

// AABB::hit (crust-rt/src/aabb.rs:24-42)
__device__ __forceinline__ bool vol_aabb_hit(const float bmin[3], const float bmax[3], V3 ro, V3 rd, float t_min, float t_max) {
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float inv_d = 1.0f / comp(rd, a);
    float t0 = (bmin[a] - comp(ro, a)) * inv_d;
    float t1 = (bmax[a] - comp(ro, a)) * inv_d;
    if (inv_d < 0.0f) { const float s = t0; t0 = t1; t1 = s; }
    t_min = rmax(t_min, t0);
    t_max = rmin(t_max, t1);
    if (t_max <= t_min) return false;
  }
  return true;
}

struct VolSpans {
  uint32_t mask;   // bit r: region r is crossed; its clipped span is sa[r * stride], sb[r * stride]
  uint32_t hetero; // bit r: ... and it is not homogeneous
  float majorant, start, end;
};

// Volumes::active_intervals (volume.rs:379-404), with the start / end folds of :423-424
__device__ __forceinline__ VolSpans vol_active_intervals(const VolRegionRec *__restrict__ regions, uint32_t n_regions, V3 ro, V3 rd,
                                                         float t_eps, float t_max, float *sa, float *sb, uint32_t stride) {
  VolSpans S;
  S.mask = S.hetero = 0u;
  S.majorant = 0.0f;
  S.start = CRT_INF;
  S.end = 0.0f;
  for (uint32_t r = 0; r < n_regions; r++) {
    const VolRegionRec &R = regions[r];
    if (R.majorant <= 0.0f) continue;
    if (!vol_aabb_hit(R.bmin, R.bmax, ro, rd, t_eps, t_max)) continue;
    float t0, t1;
    if (!vol_region_intersect(R, ro, rd, t0, t1)) continue;
    const float a = rmax(t0, t_eps), b = rmin(t1, t_max);
    if (b > a) {
      sa[r * stride] = a;
      sb[r * stride] = b;
      S.mask |= 1u << r;
      if (R.field != CRT_VOLUME_HOMOGENEOUS) S.hetero |= 1u << r;
      S.majorant += R.majorant;
      S.start = rmin(S.start, a);
      S.end = rmax(S.end, b);
    }
  }
  return S;
}

// The walk of Volumes::transmittance over spans the caller already holds (S and the columns vol_active_intervals filled):
// the renderer's kernels look at S.mask first and touch nothing where no region is crossed.
__device__ __forceinline__ uint32_t vol_transmittance_spans(const VolRegionRec *__restrict__ regions, uint32_t n_regions,
                                                            const float *__restrict__ grid, V3 ro, V3 rd, const VolSpans &S,
                                                            uint32_t seed, const float *sa, const float *sb, uint32_t stride, V3 &tr) {
  tr = splat(1.0f);
  if (S.mask == 0u || S.majorant <= 0.0f) return CRT_VOLUME_OK;
  if (S.hetero == 0u) {  // every crossed region homogeneous: the analytic product
    for (uint32_t r = 0; r < n_regions; r++) {
      if (!((S.mask >> r) & 1u)) continue;
      const VolRegionRec &R = regions[r];
      const V3 st = (v3(R.sigma_a[0], R.sigma_a[1], R.sigma_a[2]) + v3(R.sigma_s[0], R.sigma_s[1], R.sigma_s[2])) * 1.0f;
      const V3 e = st * (sb[r * stride] - sa[r * stride]);
      tr = tr * v3(exp_det(-e.x), exp_det(-e.y), exp_det(-e.z));
    }
    return CRT_VOLUME_OK;
  }
  const float majorant = S.majorant;
  float t = S.start;
  V3 w = splat(1.0f);
  for (uint32_t step = 0; step < CRT_VOLUME_MAX_STEPS; step++) {
    t += -(log_det(1.0f - vol_next_f32(seed))) / majorant;
    if (t >= S.end) { tr = w; return CRT_VOLUME_OK; }
    const V3 p = ro + rd * t;
    V3 sigma_t_x = splat(0.0f);
    for (uint32_t r = 0; r < n_regions; r++) {
      if (!((S.mask >> r) & 1u)) continue;
      if (t < sa[r * stride] || t > sb[r * stride]) continue;
      const VolRegionRec &R = regions[r];
      const float d = vol_region_density(R, grid, p);
      sigma_t_x = sigma_t_x + (v3(R.sigma_a[0], R.sigma_a[1], R.sigma_a[2]) + v3(R.sigma_s[0], R.sigma_s[1], R.sigma_s[2])) * d;
    }
    w = w * ((splat(majorant) - sigma_t_x) / majorant);
    if (max_elem(w) < 1e-5f) { tr = splat(0.0f); return CRT_VOLUME_OK; }
  }
  tr = splat(0.0f);
  return CRT_VOLUME_STEP_LIMIT;
}

// Volumes::transmittance (volume.rs:492-536). Returns the status; tr = 0 on CRT_VOLUME_STEP_LIMIT.
__device__ __forceinline__ uint32_t vol_transmittance(const VolRegionRec *__restrict__ regions, uint32_t n_regions,
                                                      const float *__restrict__ grid, V3 ro, V3 rd, float t_eps, float t_max,
                                                      uint32_t seed, float *sa, float *sb, uint32_t stride, V3 &tr) {
  const VolSpans S = vol_active_intervals(regions, n_regions, ro, rd, t_eps, t_max, sa, sb, stride);
  return vol_transmittance_spans(regions, n_regions, grid, ro, rd, S, seed, sa, sb, stride, tr);
}

struct VolEvent {
  uint32_t kind, status, n_lobes, lobe_mask;  // lobe_mask bit r: region r contributed a lobe, its normalised weight in lw[r * stride]
  float t;
  V3 p, weight, emitted;  // weight: the scatter's path weight, or the passthrough's transmittance
};

// The walk of Volumes::sample_interaction over spans the caller already holds (see vol_transmittance_spans).
__device__ __forceinline__ VolEvent vol_sample_interaction_spans(const VolRegionRec *__restrict__ regions, uint32_t n_regions,
                                                                 const float *__restrict__ grid, V3 ro, V3 rd, const VolSpans &S,
                                                                 uint32_t seed, const float *sa, const float *sb, float *lw, uint32_t stride) {
  VolEvent E;
  E.kind = CRT_VOLUME_PASSTHROUGH; E.status = CRT_VOLUME_OK; E.n_lobes = 0u; E.lobe_mask = 0u;
  E.t = 0.0f;
  E.p = splat(0.0f); E.weight = splat(1.0f); E.emitted = splat(0.0f);
  if (S.mask == 0u || S.majorant <= 0.0f) return E;
  const float majorant = S.majorant;
  float t = S.start;
  V3 w = splat(1.0f), emitted = splat(0.0f);
  for (uint32_t step = 0; step < CRT_VOLUME_MAX_STEPS; step++) {
    t += -(log_det(1.0f - vol_next_f32(seed))) / majorant;
    if (t >= S.end) { E.weight = w; E.emitted = emitted; return E; }
    const V3 p = ro + rd * t;
    V3 sigma_s_x = splat(0.0f), sigma_t_x = splat(0.0f);
    uint32_t lobe_mask = 0u;
    for (uint32_t r = 0; r < n_regions; r++) {
      if (!((S.mask >> r) & 1u)) continue;
      if (t < sa[r * stride] || t > sb[r * stride]) continue;
      const VolRegionRec &R = regions[r];
      const float d = vol_region_density(R, grid, p);
      if (d <= 0.0f) continue;
      const V3 rs = v3(R.sigma_s[0], R.sigma_s[1], R.sigma_s[2]), ra = v3(R.sigma_a[0], R.sigma_a[1], R.sigma_a[2]);
      const V3 ss = rs * d;
      sigma_s_x = sigma_s_x + ss;
      sigma_t_x = sigma_t_x + (ra + rs) * d;
      emitted = emitted + ((w * (ra * d)) * v3(R.emission[0], R.emission[1], R.emission[2])) / majorant;
      const float m = max_elem(ss);
      if (m > 0.0f) { lw[r * stride] = m; lobe_mask |= 1u << r; }
    }
    const float p_scatter = rclamp(max_elem(sigma_s_x) / majorant, 0.0f, 1.0f);
    if (vol_next_f32(seed) < p_scatter) {
      float total = 0.0f;
      uint32_t n_lobes = 0u;
      for (uint32_t r = 0; r < n_regions; r++)
        if ((lobe_mask >> r) & 1u) { total += lw[r * stride]; n_lobes++; }
      for (uint32_t r = 0; r < n_regions; r++)
        if ((lobe_mask >> r) & 1u) lw[r * stride] = lw[r * stride] / total;
      E.kind = CRT_VOLUME_SCATTER;
      E.t = t; E.p = p;
      E.weight = (w * sigma_s_x) / (majorant * p_scatter);
      E.emitted = emitted;
      E.n_lobes = n_lobes; E.lobe_mask = lobe_mask;
      return E;
    }
    w = w * ((splat(majorant) - sigma_t_x) / (majorant * (1.0f - p_scatter)));
    if (max_elem(w) < 1e-5f) { E.weight = splat(0.0f); E.emitted = emitted; return E; }
  }
  E.weight = splat(0.0f);
  E.status = CRT_VOLUME_STEP_LIMIT;
  return E;
}

// Volumes::sample_interaction (volume.rs:409-486)
__device__ __forceinline__ VolEvent vol_sample_interaction(const VolRegionRec *__restrict__ regions, uint32_t n_regions,
                                                           const float *__restrict__ grid, V3 ro, V3 rd, float t_eps, float t_max,
                                                           uint32_t seed, float *sa, float *sb, float *lw, uint32_t stride) {
  const VolSpans S = vol_active_intervals(regions, n_regions, ro, rd, t_eps, t_max, sa, sb, stride);
  return vol_sample_interaction_spans(regions, n_regions, grid, ro, rd, S, seed, sa, sb, lw, stride);
}

__device__ __forceinline__ float vol_hg_phase(float cos_theta, float g) {  // medium.rs:148-152
  const float denom = rmax(1.0f + g * g - 2.0f * g * cos_theta, 1e-6f);
  return (1.0f - g * g) / (4.0f * CRT_PI * denom * sqrtf(denom));
}

// PhaseMix::sample (volume.rs:305-316) and PhaseMix::pdf (:319-324) over the lobes a scatter left in lw (region order is
// the order the reference pushes them in), then max(pdf, 1e-6) as tracer.rs:1193-1196 takes it. wi is normalised here.
__device__ __forceinline__ void vol_phase_sample(const VolRegionRec *__restrict__ regions, uint32_t n_regions, const VolEvent &E,
                                                 const float *lw, uint32_t stride, V3 rd, float lobe_u, float hg_u, float hg_v,
                                                 V3 &dir, float &pdf) {
  const V3 wi = normalize(rd);
  float pick = lobe_u, g = 0.0f;
  bool chosen = false;
  for (uint32_t r = 0; r < n_regions; r++) {
    if (!((E.lobe_mask >> r) & 1u)) continue;
    if (chosen) continue;
    g = regions[r].g;  // the last lobe's g when none is picked
    const float wgt = lw[r * stride];
    if (pick < wgt) chosen = true;
    else pick -= wgt;
  }
  dir = sample_henyey_greenstein(wi, g, hg_u, hg_v);
  const float c = dot(wi, dir);
  float sum = 0.0f;
  for (uint32_t r = 0; r < n_regions; r++)
    if ((E.lobe_mask >> r) & 1u) sum += lw[r * stride] * vol_hg_phase(c, regions[r].g);
  pdf = rmax(sum, 1e-6f);
}

// PhaseMix::pdf (volume.rs:319-324) of a scatter's lobes at cos_theta, unclamped: the phase value volume_nee weighs a
// light sample with (tracer.rs:1054-1062).
__device__ __forceinline__ float vol_phase_pdf(const VolRegionRec *__restrict__ regions, uint32_t n_regions, const VolEvent &E,
                                               const float *lw, uint32_t stride, float cos_theta) {
  float sum = 0.0f;
  for (uint32_t r = 0; r < n_regions; r++)
    if ((E.lobe_mask >> r) & 1u) sum += lw[r * stride] * vol_hg_phase(cos_theta, regions[r].g);
  return sum;
}

}  // namespace dev
}  // namespace crt
