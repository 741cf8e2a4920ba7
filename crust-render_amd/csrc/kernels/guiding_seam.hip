// The path guiding field as callable functions: GuidingField::sample, ::pdf (field.rs:88-97) and the integrator's
// sample_bounce_direction (tracer.rs:777-826) over batches of queries, for a host integrator that keeps its own
// trace_path on crt_intersect_n / crt_occluded_n and the shading seam (shade_seam.hip) and turns on crust:pathGuiding.
//
// Thin kernels over kernels/guiding.hip.h: one query per lane, 256-thread blocks, records read and written as 16-byte
// vectors. The view of the image (pointers, counts, bounds, alpha) is a kernel argument: wave-uniform, scalar registers.
// A descent is a chain of dependent loads — at most 33 16-byte S-nodes, then at most 32 D-nodes of two 16-byte loads each
// that go out together; nothing here hides that latency but the other waves of the SIMD. The guided bounce calls the same
// mat_scatter<false> / mat_eval<false> the shading seam's kernels call. The wavefront renderer runs none of these
// kernels: its guided shade instances (pathtrace.hip, k_shade_guided) call the same guide_sample_bounce_at.
// Compile with -ffp-contract=off (dmath.hip.h).
#define CRT_GUIDING_BOUNCE
#include "guiding.hip.h"
#include "../crt_internal.h"
#include "../guiding_internal.h"

namespace crt {

using namespace dev;

namespace {

constexpr int kGuideBlock = 256;

static_assert(sizeof(CrtGuidingQuery) == 32 && sizeof(CrtGuidingResult) == 32, "crt_guiding.h record sizes");
static_assert(sizeof(CrtGuidingConfig) == 24 && sizeof(CrtGuidingSample) == 32, "crt_guiding.h record sizes");
static_assert(sizeof(CrtShadeQuery) == 80 && sizeof(CrtScatterSample) == 48, "crt.h record sizes");

// GuidingField::sample (SAMPLE) or ::pdf, with trained_at beside it
template <bool SAMPLE>
__global__ __launch_bounds__(kGuideBlock) void k_guide_query(GuideView V, const CrtGuidingQuery *__restrict__ qs, size_t n,
                                                            CrtGuidingResult *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kGuideBlock + threadIdx.x;
  if (i >= n) return;
  const float4 *w = reinterpret_cast<const float4 *>(qs + i);
  const float4 a = w[0], b = w[1];
  const V3 pos = v3(a.x, a.y, a.z);
  V3 dir = splat(0.0f);
  float pdf = 0.0f;
  bool some = true, trained = false;
  if (SAMPLE) some = guide_field_sample(V, pos, a.w, b.w, dir, pdf, trained);
  else pdf = guide_field_pdf(V, pos, v3(b.x, b.y, b.z), trained);
  float4 *o = reinterpret_cast<float4 *>(out + i);
  o[0] = make_float4(dir.x, dir.y, dir.z, pdf);
  o[1] = make_float4(__uint_as_float(some ? 1u : 0u), __uint_as_float(trained ? 1u : 0u), 0.0f, 0.0f);
}

// sample_bounce_direction (tracer.rs:777-826); the query record is shade_seam.hip's
__global__ __launch_bounds__(kGuideBlock) void k_guide_scatter(GuideView V, const CrtMaterial *mats, uint32_t n_mats, const CrtShadeQuery *qs,
                                                              size_t n, CrtScatterSample *out) {
  __shared__ uint32_t sobol_tab[kSobolLdsWords];
  sobol_tables_init(sobol_tab);  // ends with a barrier
  const size_t i = (size_t)blockIdx.x * kGuideBlock + threadIdx.x;
  if (i >= n) return;
  const float4 *w = reinterpret_cast<const float4 *>(qs + i);
  const float4 a = w[0], b = w[1], c = w[2];
  const uint4 e = reinterpret_cast<const uint4 *>(qs + i)[4];
  const V3 rd = v3(a.x, a.y, a.z);
  const uint32_t material = __float_as_uint(a.w);
  HitRec rec;
  rec.p = v3(b.x, b.y, b.z); rec.t = b.w;
  rec.normal = v3(c.x, c.y, c.z); rec.front_face = __float_as_uint(c.w) != 0;
  Scatter sc;
  sc.origin = sc.dir = sc.value = splat(0.0f); sc.pdf = 0.0f; sc.delta = false; sc.medium = false;
  uint32_t flags = 0;
  bool some = false;
  if (material < n_mats) some = guide_sample_bounce(V, mats[material], rd, rec, Sampler{e.x, e.y}, sc, flags, sobol_tab);
  if (!some) { sc.origin = sc.dir = sc.value = splat(0.0f); sc.pdf = 0.0f; sc.delta = false; sc.medium = false; }
  float4 *o = reinterpret_cast<float4 *>(out + i);
  o[0] = make_float4(sc.origin.x, sc.origin.y, sc.origin.z, __uint_as_float(some ? 1u : 0u));
  o[1] = make_float4(sc.dir.x, sc.dir.y, sc.dir.z, sc.pdf);
  o[2] = make_float4(sc.value.x, sc.value.y, sc.value.z, __uint_as_float((sc.delta ? 1u : 0u) | (sc.medium ? 2u : 0u) | flags));
}

// 1: nothing to do | CRT_OK | an error — before a device is touched
int guide_args(const CrtGuiding *g, const void *queries, size_t n, const void *out) {
  if (!g) return CRT_ERR_BAD_ARG;
  if (n == 0) return 1;
  if (!queries || !out) return CRT_ERR_BAD_ARG;
  if (n > 0xffffffffull * kGuideBlock) return CRT_ERR_BAD_ARG;
  return CRT_OK;
}
unsigned guide_grid(size_t n) { return (unsigned)((n + kGuideBlock - 1) / kGuideBlock); }
int guide_done() { return CRT_HIP_OK(hipGetLastError()) ? CRT_OK : CRT_ERR_NO_DEVICE; }

template <bool SAMPLE>
int guide_query(CrtGuiding *g, const CrtGuidingQuery *d_queries, size_t n, CrtGuidingResult *d_out, void *stream) {
  int rc = guide_args(g, d_queries, n, d_out);
  if (rc != CRT_OK) return rc > 0 ? CRT_OK : rc;
  GuideView V;
  rc = guiding_device(g, V);
  if (rc != CRT_OK) return rc;
  hipLaunchKernelGGL((k_guide_query<SAMPLE>), dim3(guide_grid(n)), dim3(kGuideBlock), 0, (hipStream_t)stream, V, d_queries, n, d_out);
  return guide_done();
}

}  // namespace
}  // namespace crt

using namespace crt;

extern "C" {

int crt_guiding_sample_n(CrtGuiding *g, const CrtGuidingQuery *d_queries, size_t n, CrtGuidingResult *d_out, void *stream) {
  return guide_query<true>(g, d_queries, n, d_out, stream);
}
int crt_guiding_pdf_n(CrtGuiding *g, const CrtGuidingQuery *d_queries, size_t n, CrtGuidingResult *d_out, void *stream) {
  return guide_query<false>(g, d_queries, n, d_out, stream);
}
int crt_material_scatter_guided_n(CrtGuiding *g, const CrtMaterial *d_materials, size_t n_materials, const CrtShadeQuery *d_queries,
                                  size_t n, CrtScatterSample *d_out, void *stream) {
  int rc = guide_args(g, d_queries, n, d_out);
  if (rc != CRT_OK) return rc > 0 ? CRT_OK : rc;
  if ((n_materials && !d_materials) || n_materials > 0xffffffffull) return CRT_ERR_BAD_ARG;
  GuideView V;
  rc = guiding_device(g, V);
  if (rc != CRT_OK) return rc;
  hipLaunchKernelGGL(k_guide_scatter, dim3(guide_grid(n)), dim3(kGuideBlock), 0, (hipStream_t)stream, V, d_materials, (uint32_t)n_materials,
                     d_queries, n, d_out);
  return guide_done();
}

}  // extern "C"
