// The volume aggregate as callable functions: VolumeRegion::density, Volumes::transmittance and
// Volumes::sample_interaction (volume.rs:234-242, :492-536, :409-486) over batches of queries, for a host integrator
// that keeps its own trace_path on crt_intersect_n / crt_occluded_n and the shading seam (shade_seam.hip).
//
// Thin kernels over kernels/volume.hip.h: one query per lane, 256-thread blocks, records read and written as 16-byte
// vectors. The region records arrive through a const __restrict__ kernel argument and are indexed by the uniform region
// loop (scalar loads); a lane's spans and lobe weights are LDS columns [region][thread] — 24 KB a block in the sample
// kernel, 16 KB in the transmittance kernel — because a runtime-indexed private array would live in scratch
// (profiles/volume_isa_resources.txt has the rows). The wavefront renderer runs the same header in kernels of its own
// (pathtrace.hip: k_volume, k_shadow_volume), not these.
// Compile with -ffp-contract=off (dmath.hip.h).
#include "volume.hip.h"
#include "../crt_internal.h"

namespace crt {

using namespace dev;

namespace {

constexpr int kVolBlock = 256;

static_assert(sizeof(CrtVolumeRegion) == 152 && sizeof(CrtVolumeQuery) == 48, "crt.h record sizes");
static_assert(sizeof(CrtVolumeTransmittance) == 16 && sizeof(CrtVolumeEvent) == 144, "crt.h record sizes");

struct VQuery { V3 o, d; float t_eps, t_max; uint32_t seed; };
__device__ __forceinline__ VQuery load_vquery(const CrtVolumeQuery *q) {
  const float4 *w = reinterpret_cast<const float4 *>(q);
  const float4 a = w[0], b = w[1], c = w[2];
  VQuery o;
  o.o = v3(a.x, a.y, a.z); o.t_eps = a.w;
  o.d = v3(b.x, b.y, b.z); o.t_max = b.w;
  o.seed = __float_as_uint(c.x);
  return o;
}

__global__ __launch_bounds__(kVolBlock) void k_vol_density(const VolRegionRec *__restrict__ regions, uint32_t region,
                                                          const float *__restrict__ grid, const float *__restrict__ points, size_t n,
                                                          float *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kVolBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = vol_region_density(regions[region], grid, v3(points[3 * i], points[3 * i + 1], points[3 * i + 2]));
}

__global__ __launch_bounds__(kVolBlock) void k_vol_transmittance(const VolRegionRec *__restrict__ regions, uint32_t n_regions,
                                                                const float *__restrict__ grid, const CrtVolumeQuery *__restrict__ qs,
                                                                size_t n, CrtVolumeTransmittance *__restrict__ out) {
  __shared__ float span_a[kVolMaxRegions][kVolBlock], span_b[kVolMaxRegions][kVolBlock];
  const size_t i = (size_t)blockIdx.x * kVolBlock + threadIdx.x;
  if (i >= n) return;  // no barrier below: a lane only ever touches its own column
  const VQuery q = load_vquery(qs + i);
  V3 tr;
  const uint32_t status = vol_transmittance(regions, n_regions, grid, q.o, q.d, q.t_eps, q.t_max, q.seed, &span_a[0][threadIdx.x],
                                            &span_b[0][threadIdx.x], kVolBlock, tr);
  *reinterpret_cast<float4 *>(out + i) = make_float4(tr.x, tr.y, tr.z, __uint_as_float(status));
}

__global__ __launch_bounds__(kVolBlock) void k_vol_sample(const VolRegionRec *__restrict__ regions, uint32_t n_regions,
                                                         const float *__restrict__ grid, const CrtVolumeQuery *__restrict__ qs,
                                                         const float *__restrict__ phase_u, size_t n, CrtVolumeEvent *__restrict__ out) {
  __shared__ float span_a[kVolMaxRegions][kVolBlock], span_b[kVolMaxRegions][kVolBlock], lobe_w[kVolMaxRegions][kVolBlock];
  const size_t i = (size_t)blockIdx.x * kVolBlock + threadIdx.x;
  if (i >= n) return;  // no barrier below: a lane only ever touches its own column
  const VQuery q = load_vquery(qs + i);
  float *lw = &lobe_w[0][threadIdx.x];
  const VolEvent E = vol_sample_interaction(regions, n_regions, grid, q.o, q.d, q.t_eps, q.t_max, q.seed, &span_a[0][threadIdx.x],
                                            &span_b[0][threadIdx.x], lw, kVolBlock);
  V3 dir = splat(0.0f);
  float pdf = 0.0f;
  const bool scatter = E.kind == CRT_VOLUME_SCATTER;
  if (scatter && phase_u) vol_phase_sample(regions, n_regions, E, lw, kVolBlock, q.d, phase_u[3 * i], phase_u[3 * i + 1], phase_u[3 * i + 2], dir, pdf);
  const bool limit = E.status != CRT_VOLUME_OK;
  const V3 wgt = limit ? splat(0.0f) : E.weight, em = limit ? splat(0.0f) : E.emitted;
  float4 *w = reinterpret_cast<float4 *>(out + i);
  w[0] = make_float4(E.p.x, E.p.y, E.p.z, E.t);
  w[1] = make_float4(wgt.x, wgt.y, wgt.z, __uint_as_float(E.kind));
  w[2] = make_float4(em.x, em.y, em.z, __uint_as_float(E.n_lobes));
  w[3] = make_float4(dir.x, dir.y, dir.z, pdf);
  w[4] = w[5] = w[6] = w[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  w[8] = make_float4(__uint_as_float(E.status), 0.0f, 0.0f, 0.0f);
  if (scatter) {  // the lobes in the order the reference pushes them: region order
    float2 *lobes = reinterpret_cast<float2 *>(w + 4);
    uint32_t k = 0;
    for (uint32_t r = 0; r < n_regions; r++)
      if ((E.lobe_mask >> r) & 1u) lobes[k++] = make_float2(lw[r * kVolBlock], regions[r].g);
  }
}

int vol_args(const CrtVolumes *v, const void *queries, size_t n, const void *out) {
  if (!v) return CRT_ERR_BAD_ARG;
  if (n == 0) return 1;  // nothing to do
  if (!queries || !out) return CRT_ERR_BAD_ARG;
  return CRT_OK;
}
unsigned vol_grid(size_t n) { return (unsigned)((n + kVolBlock - 1) / kVolBlock); }
int vol_done() { return CRT_HIP_OK(hipGetLastError()) ? CRT_OK : CRT_ERR_NO_DEVICE; }

}  // namespace
}  // namespace crt

using namespace crt;

extern "C" {

int crt_volumes_density_n(CrtVolumes *v, uint32_t region, const float *d_points, size_t n, float *d_density, void *stream) {
  int rc = vol_args(v, d_points, n, d_density);
  if (rc == CRT_OK || rc > 0)
    if (region >= volumes_region_count(v)) { set_error_text("crt_volumes_density_n: region %u of %u", region, volumes_region_count(v)); return CRT_ERR_BAD_ARG; }
  if (rc != CRT_OK) return rc > 0 ? CRT_OK : rc;
  if (n > 0xffffffffull * kVolBlock) return CRT_ERR_BAD_ARG;
  VolumesView V;
  rc = volumes_device(v, V);
  if (rc != CRT_OK) return rc;
  hipLaunchKernelGGL(k_vol_density, dim3(vol_grid(n)), dim3(kVolBlock), 0, (hipStream_t)stream, V.regions, region, V.grid, d_points, n, d_density);
  return vol_done();
}

int crt_volumes_transmittance_n(CrtVolumes *v, const CrtVolumeQuery *d_queries, size_t n, CrtVolumeTransmittance *d_out, void *stream) {
  int rc = vol_args(v, d_queries, n, d_out);
  if (rc != CRT_OK) return rc > 0 ? CRT_OK : rc;
  if (n > 0xffffffffull * kVolBlock) return CRT_ERR_BAD_ARG;
  VolumesView V;
  rc = volumes_device(v, V);
  if (rc != CRT_OK) return rc;
  hipLaunchKernelGGL(k_vol_transmittance, dim3(vol_grid(n)), dim3(kVolBlock), 0, (hipStream_t)stream, V.regions, V.n_regions, V.grid, d_queries, n, d_out);
  return vol_done();
}

int crt_volumes_sample_n(CrtVolumes *v, const CrtVolumeQuery *d_queries, const float *d_phase_u, size_t n, CrtVolumeEvent *d_events,
                         void *stream) {
  int rc = vol_args(v, d_queries, n, d_events);
  if (rc != CRT_OK) return rc > 0 ? CRT_OK : rc;
  if (n > 0xffffffffull * kVolBlock) return CRT_ERR_BAD_ARG;
  VolumesView V;
  rc = volumes_device(v, V);
  if (rc != CRT_OK) return rc;
  hipLaunchKernelGGL(k_vol_sample, dim3(vol_grid(n)), dim3(kVolBlock), 0, (hipStream_t)stream, V.regions, V.n_regions, V.grid, d_queries, d_phase_u, n,
                     d_events);
  return vol_done();
}

}  // extern "C"
