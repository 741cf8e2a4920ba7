// CPU twin of the volume aggregate's device functions (tests only): kernels/volume.hip.h — the SAME source the seam
// kernels include — compiled as host C++ behind the HIP stand-in header profiles/host_shade/hip/hip_runtime.h and
// exported over arrays, so tests/test_volumes.py can compare it with the numpy restatement (tests/volume_ref.py) bit for
// bit, and so that restatement takes its log / exp / sincos from the device source. `image` is the byte image
// crt_volumes_image hands out (host memory). A lane's span and lobe columns are plain arrays here (stride 1).
// Build: tests/volume_ref.py (g++ -O1 -ffp-contract=off -shared, as tests/env_ref.py builds env_host.cpp).
#include <cstddef>
#include <cstdint>

#include "volume.hip.h"

using namespace crt::dev;

namespace {
struct View { const VolRegionRec *regions; const float *grid; uint32_t n; };
View view(const void *image) {
  const unsigned char *im = static_cast<const unsigned char *>(image);
  const VolHeader *h = reinterpret_cast<const VolHeader *>(im);
  return View{reinterpret_cast<const VolRegionRec *>(im + h->off_regions), reinterpret_cast<const float *>(im + h->off_grid), h->n_regions};
}
}  // namespace

extern "C" {

void host_vol_log_n(const float *x, size_t n, float *o) { for (size_t i = 0; i < n; i++) o[i] = log_det(x[i]); }
void host_vol_exp_n(const float *x, size_t n, float *o) { for (size_t i = 0; i < n; i++) o[i] = exp_det(x[i]); }
void host_vol_sincos_n(const float *x, size_t n, float *s, float *c) { for (size_t i = 0; i < n; i++) sincos_det(x[i], s[i], c[i]); }

void host_vol_density_n(const void *image, uint32_t region, const float *p, size_t n, float *o) {
  const View V = view(image);
  for (size_t i = 0; i < n; i++) o[i] = vol_region_density(V.regions[region], V.grid, v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]));
}
// VolumeRegion::intersect: out = some (1.0 / 0.0), t0, t1 (zeros for None); rays = 6 floats (origin, direction)
void host_vol_intersect_n(const void *image, uint32_t region, const float *rays, size_t n, float *out) {
  const View V = view(image);
  for (size_t i = 0; i < n; i++) {
    const float *r = rays + 6 * i;
    float t0, t1;
    const bool some = vol_region_intersect(V.regions[region], v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]), t0, t1);
    out[3 * i] = some ? 1.0f : 0.0f; out[3 * i + 1] = some ? t0 : 0.0f; out[3 * i + 2] = some ? t1 : 0.0f;
  }
}
// Volumes::active_intervals: queries = CrtVolumeQuery records; out per query = mask (u32 bits), majorant, then 8 x (a, b)
// (zeros for regions not crossed): 18 floats
void host_vol_intervals_n(const void *image, const CrtVolumeQuery *q, size_t n, float *out) {
  const View V = view(image);
  for (size_t i = 0; i < n; i++) {
    float sa[kVolMaxRegions] = {}, sb[kVolMaxRegions] = {};
    const VolSpans S = vol_active_intervals(V.regions, V.n, v3(q[i].origin[0], q[i].origin[1], q[i].origin[2]),
                                            v3(q[i].direction[0], q[i].direction[1], q[i].direction[2]), q[i].t_eps, q[i].t_max, sa, sb, 1);
    float *o = out + 18 * i;
    o[0] = __uint_as_float(S.mask); o[1] = S.majorant;
    for (uint32_t r = 0; r < kVolMaxRegions; r++) {
      const bool on = (S.mask >> r) & 1u;
      o[2 + 2 * r] = on ? sa[r] : 0.0f; o[3 + 2 * r] = on ? sb[r] : 0.0f;
    }
  }
}
void host_vol_transmittance_n(const void *image, const CrtVolumeQuery *q, size_t n, CrtVolumeTransmittance *out) {
  const View V = view(image);
  for (size_t i = 0; i < n; i++) {
    float sa[kVolMaxRegions] = {}, sb[kVolMaxRegions] = {};
    V3 tr;
    out[i].status = vol_transmittance(V.regions, V.n, V.grid, v3(q[i].origin[0], q[i].origin[1], q[i].origin[2]),
                                      v3(q[i].direction[0], q[i].direction[1], q[i].direction[2]), q[i].t_eps, q[i].t_max, q[i].seed, sa, sb, 1, tr);
    out[i].transmittance[0] = tr.x; out[i].transmittance[1] = tr.y; out[i].transmittance[2] = tr.z;
  }
}
// the record k_vol_sample writes, field by field
void host_vol_sample_n(const void *image, const CrtVolumeQuery *q, const float *phase_u, size_t n, CrtVolumeEvent *out) {
  const View V = view(image);
  for (size_t i = 0; i < n; i++) {
    float sa[kVolMaxRegions] = {}, sb[kVolMaxRegions] = {}, lw[kVolMaxRegions] = {};
    const V3 ro = v3(q[i].origin[0], q[i].origin[1], q[i].origin[2]), rd = v3(q[i].direction[0], q[i].direction[1], q[i].direction[2]);
    const VolEvent E = vol_sample_interaction(V.regions, V.n, V.grid, ro, rd, q[i].t_eps, q[i].t_max, q[i].seed, sa, sb, lw, 1);
    CrtVolumeEvent &o = out[i];
    std::memset(&o, 0, sizeof(o));
    V3 dir = splat(0.0f);
    float pdf = 0.0f;
    const bool scatter = E.kind == CRT_VOLUME_SCATTER;
    if (scatter && phase_u) vol_phase_sample(V.regions, V.n, E, lw, 1, rd, phase_u[3 * i], phase_u[3 * i + 1], phase_u[3 * i + 2], dir, pdf);
    o.p[0] = E.p.x; o.p[1] = E.p.y; o.p[2] = E.p.z; o.t = E.t;
    o.weight[0] = E.weight.x; o.weight[1] = E.weight.y; o.weight[2] = E.weight.z; o.kind = E.kind;
    o.emitted[0] = E.emitted.x; o.emitted[1] = E.emitted.y; o.emitted[2] = E.emitted.z; o.n_lobes = E.n_lobes;
    o.dir[0] = dir.x; o.dir[1] = dir.y; o.dir[2] = dir.z; o.pdf = pdf;
    o.status = E.status;
    if (scatter) {
      uint32_t k = 0;
      for (uint32_t r = 0; r < V.n; r++)
        if ((E.lobe_mask >> r) & 1u) { o.lobes[k][0] = lw[r]; o.lobes[k][1] = V.regions[r].g; k++; }
    }
  }
}
// PhaseMix::pdf of explicit lobes (volume.rs:319-324) and hg_phase (medium.rs:148-152)
void host_vol_hg_phase_n(const float *c, const float *g, size_t n, float *o) { for (size_t i = 0; i < n; i++) o[i] = vol_hg_phase(c[i], g[i]); }

}  // extern "C"
