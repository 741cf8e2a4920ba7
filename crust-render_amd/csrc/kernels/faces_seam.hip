// Per-face textures as callable functions: World::intersect's face lookup (rt_world.rs:207-232), PtexTexture::eval
// (crust-render main.rs:277-314) and Material::scatter_importance / eval with the texel in the place of base_color
// (openpbr.rs:1011-1024, :1162-1180), over batches of queries — for a host integrator that keeps its own trace_path on
// crt_intersect_n / crt_occluded_n and the shading seam (shade_seam.hip).
//
// Thin kernels over kernels/faces.hip.h and the general shading instance of shade.hip.h: one query per lane, 256-thread
// blocks, records read and written as 16-byte vectors where their size allows. The textured material kernels run ONE
// instance of mat_scatter / mat_eval, over MatFace: a query without a texture or without a face carries the record's own
// base colour in the three registers, which gives the bits of the untextured call (the same operations on the same
// values). The 60-dword material record is never copied per lane.
// Compile with -ffp-contract=off (dmath.hip.h).
#include "shade.hip.h"
#include "faces.hip.h"
#include "../crt_internal.h"
#include "../face_textures_internal.h"

namespace crt {

using namespace dev;

namespace {

constexpr int kFaceBlock = 256;

static_assert(sizeof(CrtRayHit) == 40 && sizeof(CrtFaceCoord) == 16, "record sizes");
static_assert(sizeof(CrtShadeQuery) == 80 && sizeof(CrtScatterSample) == 48 && sizeof(CrtBsdfEval) == 32, "crt.h record sizes");

__global__ __launch_bounds__(kFaceBlock) void k_face_resolve(FaceView F, const CrtRayHit *__restrict__ hits, size_t n,
                                                            CrtFaceCoord *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kFaceBlock + threadIdx.x;
  if (i >= n) return;
  const CrtRayHit &h = hits[i];  // 40 bytes, u at byte 20: four scalar loads
  FaceCoord c{kNoFace, 0.0f, 0.0f};
  if (h.geom_id != CRT_INVALID_ID) c = face_resolve(F, h.geom_id, h.prim_id, h.u, h.v);
  *reinterpret_cast<uint4 *>(out + i) = make_uint4(c.face, __float_as_uint(c.u), __float_as_uint(c.v), 0u);
}

__global__ __launch_bounds__(kFaceBlock) void k_face_eval(FaceView F, uint32_t texture, const CrtFaceCoord *__restrict__ coords, size_t n,
                                                         float *__restrict__ rgb) {
  const size_t i = (size_t)blockIdx.x * kFaceBlock + threadIdx.x;
  if (i >= n) return;
  const uint4 c = *reinterpret_cast<const uint4 *>(coords + i);
  const V3 t = face_texture_eval(F, texture, c.x, __uint_as_float(c.y), __uint_as_float(c.z));
  rgb[3 * i] = t.x; rgb[3 * i + 1] = t.y; rgb[3 * i + 2] = t.z;
}

struct Query { V3 rd; uint32_t material; HitRec rec; V3 wi; Sampler dom; };
__device__ __forceinline__ Query load_query(const CrtShadeQuery *q) {
  const float4 *w = reinterpret_cast<const float4 *>(q);
  const float4 a = w[0], b = w[1], c = w[2], d = w[3];
  const uint4 e = reinterpret_cast<const uint4 *>(q)[4];
  Query o;
  o.rd = v3(a.x, a.y, a.z); o.material = __float_as_uint(a.w);
  o.rec.p = v3(b.x, b.y, b.z); o.rec.t = b.w;
  o.rec.normal = v3(c.x, c.y, c.z); o.rec.front_face = __float_as_uint(c.w) != 0;
  o.wi = v3(d.x, d.y, d.z);
  o.dom = Sampler{e.x, e.y};
  return o;
}
// The base colour a query shades with: the texel where its material has a texture and its hit a face, else the record's.
__device__ __forceinline__ V3 query_base_color(const FaceView &F, const CrtMaterial &m, uint32_t material, const CrtFaceCoord *coord) {
  const uint4 c = *reinterpret_cast<const uint4 *>(coord);
  const uint32_t tex = material < F.n_materials ? F.material_texture[material] : kFaceNone;
  if (tex == kFaceNone || c.x == kNoFace) return ld3(m.base_color);
  return face_texture_eval(F, tex, c.x, __uint_as_float(c.y), __uint_as_float(c.z));
}

// k_seam_scatter (shade_seam.hip) over MatFace
__global__ __launch_bounds__(kFaceBlock) void k_face_scatter(FaceView F, const CrtMaterial *mats, uint32_t n_mats, const CrtShadeQuery *qs,
                                                            const CrtFaceCoord *coords, size_t n, CrtScatterSample *out) {
  __shared__ uint32_t sobol_tab[kSobolLdsWords];
  sobol_tables_init(sobol_tab);  // ends with a barrier
  const size_t i = (size_t)blockIdx.x * kFaceBlock + threadIdx.x;
  if (i >= n) return;
  const Query q = load_query(qs + i);
  Scatter sc;
  sc.origin = sc.dir = sc.value = splat(0.0f); sc.pdf = 0.0f; sc.delta = false; sc.medium = false;
  bool some = false;
  if (q.material < n_mats) {
    const CrtMaterial &m = mats[q.material];
    const MatFace mv{m, BaseTexel{query_base_color(F, m, q.material, coords + i)}};
    some = mat_scatter<false, MatFace>(mv, q.rd, q.rec, q.dom, sc, sobol_tab);
    if (some && sc.medium) {
      DevMedium med;
      medium_from_material(m, med);
      sc.medium = med.present != 0;
    }
  }
  if (!some) { sc.origin = sc.dir = sc.value = splat(0.0f); sc.pdf = 0.0f; sc.delta = false; sc.medium = false; }
  float4 *w = reinterpret_cast<float4 *>(out + i);
  w[0] = make_float4(sc.origin.x, sc.origin.y, sc.origin.z, __uint_as_float(some ? 1u : 0u));
  w[1] = make_float4(sc.dir.x, sc.dir.y, sc.dir.z, sc.pdf);
  w[2] = make_float4(sc.value.x, sc.value.y, sc.value.z, __uint_as_float((sc.delta ? 1u : 0u) | (sc.medium ? 2u : 0u)));
}

// k_seam_eval (shade_seam.hip) over MatFace
__global__ __launch_bounds__(kFaceBlock) void k_face_mat_eval(FaceView F, const CrtMaterial *mats, uint32_t n_mats, const CrtShadeQuery *qs,
                                                             const CrtFaceCoord *coords, size_t n, CrtBsdfEval *out) {
  const size_t i = (size_t)blockIdx.x * kFaceBlock + threadIdx.x;
  if (i >= n) return;
  const Query q = load_query(qs + i);
  V3 value = splat(0.0f);
  float pdf = 0.0f;
  bool some = false;
  if (q.material < n_mats) {
    const CrtMaterial &m = mats[q.material];
    const MatFace mv{m, BaseTexel{query_base_color(F, m, q.material, coords + i)}};
    some = mat_eval<false, MatFace>(mv, q.rd, q.rec, q.wi, value, pdf);
  }
  if (!some) { value = splat(0.0f); pdf = 0.0f; }
  float4 *w = reinterpret_cast<float4 *>(out + i);
  w[0] = make_float4(value.x, value.y, value.z, pdf);
  w[1] = make_float4(__uint_as_float(some ? 1u : 0u), 0.0f, 0.0f, 0.0f);
}

// CRT_OK to launch, 1 for nothing to do, or the error
int face_args(const CrtFaceTextures *ft, const void *in, size_t n, const void *out) {
  if (!ft) return CRT_ERR_BAD_ARG;
  if (n == 0) return 1;
  if (!in || !out || n > 0xffffffffull * kFaceBlock) return CRT_ERR_BAD_ARG;
  return CRT_OK;
}
unsigned face_grid(size_t n) { return (unsigned)((n + kFaceBlock - 1) / kFaceBlock); }
int face_done() { return CRT_HIP_OK(hipGetLastError()) ? CRT_OK : CRT_ERR_NO_DEVICE; }

}  // namespace
}  // namespace crt

using namespace crt;

extern "C" {

int crt_face_resolve_n(CrtFaceTextures *ft, const CrtRayHit *d_hits, size_t n, CrtFaceCoord *d_coords, void *stream) {
  int rc = face_args(ft, d_hits, n, d_coords);
  if (rc != CRT_OK) return rc > 0 ? CRT_OK : rc;
  FaceView F;
  rc = face_textures_device(ft, F);
  if (rc != CRT_OK) return rc;
  hipLaunchKernelGGL(k_face_resolve, dim3(face_grid(n)), dim3(kFaceBlock), 0, (hipStream_t)stream, F, d_hits, n, d_coords);
  return face_done();
}

int crt_face_texture_eval_n(CrtFaceTextures *ft, uint32_t texture, const CrtFaceCoord *d_coords, size_t n, float *d_rgb, void *stream) {
  int rc = face_args(ft, d_coords, n, d_rgb);
  if (rc == CRT_OK || rc > 0) {
    const uint32_t have = face_textures_texture_count(ft);
    if (texture >= have) { set_error_text("crt_face_texture_eval_n: texture %u of %u", texture, have); return CRT_ERR_BAD_ARG; }
  }
  if (rc != CRT_OK) return rc > 0 ? CRT_OK : rc;
  FaceView F;
  rc = face_textures_device(ft, F);
  if (rc != CRT_OK) return rc;
  hipLaunchKernelGGL(k_face_eval, dim3(face_grid(n)), dim3(kFaceBlock), 0, (hipStream_t)stream, F, texture, d_coords, n, d_rgb);
  return face_done();
}

int crt_material_scatter_faces_n(CrtFaceTextures *ft, const CrtMaterial *d_materials, size_t n_materials, const CrtShadeQuery *d_queries,
                                 const CrtFaceCoord *d_coords, size_t n, CrtScatterSample *d_out, void *stream) {
  int rc = face_args(ft, d_queries, n, d_out);
  if (rc != CRT_OK) return rc > 0 ? CRT_OK : rc;
  if (!d_coords || (n_materials && !d_materials) || n_materials > 0xffffffffull) return CRT_ERR_BAD_ARG;
  FaceView F;
  rc = face_textures_device(ft, F);
  if (rc != CRT_OK) return rc;
  hipLaunchKernelGGL(k_face_scatter, dim3(face_grid(n)), dim3(kFaceBlock), 0, (hipStream_t)stream, F, d_materials, (uint32_t)n_materials,
                     d_queries, d_coords, n, d_out);
  return face_done();
}

int crt_material_eval_faces_n(CrtFaceTextures *ft, const CrtMaterial *d_materials, size_t n_materials, const CrtShadeQuery *d_queries,
                              const CrtFaceCoord *d_coords, size_t n, CrtBsdfEval *d_out, void *stream) {
  int rc = face_args(ft, d_queries, n, d_out);
  if (rc != CRT_OK) return rc > 0 ? CRT_OK : rc;
  if (!d_coords || (n_materials && !d_materials) || n_materials > 0xffffffffull) return CRT_ERR_BAD_ARG;
  FaceView F;
  rc = face_textures_device(ft, F);
  if (rc != CRT_OK) return rc;
  hipLaunchKernelGGL(k_face_mat_eval, dim3(face_grid(n)), dim3(kFaceBlock), 0, (hipStream_t)stream, F, d_materials, (uint32_t)n_materials,
                     d_queries, d_coords, n, d_out);
  return face_done();
}

}  // extern "C"
