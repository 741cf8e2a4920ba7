// CPU twin of kernels/faces_seam.hip (tests only): kernels/faces.hip.h and the MatFace view of kernels/shade.hip.h — the
// SAME source the kernels include — compiled as host C++ behind the HIP stand-in header
// profiles/host_shade/hip/hip_runtime.h and exported over arrays, so tests/test_face_textures.py can compare it with the
// numpy restatement (tests/face_ref.py) and with the untextured drivers, bit for bit. `image` is the byte image
// crt_face_textures_image hands out (host memory).
// Build: tests/test_face_textures.py (g++ -O1 -ffp-contract=off -shared, as test_shading_seam_host.py builds seam_host.cpp).
#include <cstddef>
#include <cstring>

#include "shade.hip.h"
#include "faces.hip.h"
#include "crt_face_textures.h"

using namespace crt;
using namespace crt::dev;

namespace {
FaceView view(const void *image) {
  const unsigned char *im = static_cast<const unsigned char *>(image);
  const CrtFaceTexturesHeader *h = reinterpret_cast<const CrtFaceTexturesHeader *>(im);
  FaceView F;
  F.textures = reinterpret_cast<const FaceTexRec *>(im + h->off_textures);
  F.faces = reinterpret_cast<const FaceRectRec *>(im + h->off_faces);
  F.maps = reinterpret_cast<const FaceMapRec *>(im + h->off_maps);
  F.map_faces = reinterpret_cast<const uint32_t *>(im + h->off_map_faces);
  F.map_slices = im + h->off_map_slices;
  F.geoms = reinterpret_cast<const uint32_t *>(im + h->off_geoms);
  F.material_texture = reinterpret_cast<const uint32_t *>(im + h->off_material_texture);
  F.texels = reinterpret_cast<const float4 *>(im + h->off_texels);
  F.n_textures = h->n_textures; F.n_maps = h->n_maps; F.n_geoms = h->n_geoms; F.n_materials = h->n_materials;
  return F;
}
uint32_t g_tab[kSobolLdsWords];
bool g_tab_ready = false;
const uint32_t *sobol_tab() {
  if (!g_tab_ready) { sobol_tables_init(g_tab); g_tab_ready = true; }
  return g_tab;
}
HitRec rec_of(const CrtShadeQuery &q) {
  HitRec r;
  r.p = v3(q.p[0], q.p[1], q.p[2]); r.normal = v3(q.normal[0], q.normal[1], q.normal[2]); r.t = q.t;
  r.front_face = q.front_face != 0;
  return r;
}
void put(float d[3], V3 a) { d[0] = a.x; d[1] = a.y; d[2] = a.z; }
// as query_base_color (faces_seam.hip)
V3 base_of(const FaceView &F, const CrtMaterial &m, uint32_t material, const CrtFaceCoord &c) {
  const uint32_t tex = material < F.n_materials ? F.material_texture[material] : kFaceNone;
  if (tex == kFaceNone || c.face_id == kNoFace) return ld3(m.base_color);
  return face_texture_eval(F, tex, c.face_id, c.u, c.v);
}
}  // namespace

extern "C" {

void host_face_resolve_n(const void *image, const CrtRayHit *hits, size_t n, CrtFaceCoord *out) {
  const FaceView F = view(image);
  for (size_t i = 0; i < n; i++) {
    FaceCoord c{kNoFace, 0.0f, 0.0f};
    if (hits[i].geom_id != CRT_INVALID_ID) c = face_resolve(F, hits[i].geom_id, hits[i].prim_id, hits[i].u, hits[i].v);
    out[i].face_id = c.face; out[i].u = c.u; out[i].v = c.v; out[i]._pad = 0;
  }
}
void host_face_eval_n(const void *image, uint32_t texture, const CrtFaceCoord *coords, size_t n, float *rgb) {
  const FaceView F = view(image);
  for (size_t i = 0; i < n; i++) put(rgb + 3 * i, face_texture_eval(F, texture, coords[i].face_id, coords[i].u, coords[i].v));
}
void host_face_scatter_n(const void *image, const CrtMaterial *mats, size_t n_mats, const CrtShadeQuery *qs, const CrtFaceCoord *coords,
                         size_t n, CrtScatterSample *out) {
  const FaceView F = view(image);
  const uint32_t *tab = sobol_tab();
  for (size_t i = 0; i < n; i++) {
    std::memset(&out[i], 0, sizeof out[i]);
    if (qs[i].material >= n_mats) continue;
    const CrtMaterial &m = mats[qs[i].material];
    const MatFace mv{m, BaseTexel{base_of(F, m, qs[i].material, coords[i])}};
    Scatter sc;
    if (!mat_scatter<false, MatFace>(mv, v3(qs[i].ray_dir[0], qs[i].ray_dir[1], qs[i].ray_dir[2]), rec_of(qs[i]),
                                     Sampler{qs[i].sampler_pattern, qs[i].sampler_index}, sc, tab)) continue;
    if (sc.medium) { DevMedium med; medium_from_material(m, med); sc.medium = med.present != 0; }
    put(out[i].origin, sc.origin); put(out[i].dir, sc.dir); put(out[i].value, sc.value);
    out[i].some = 1; out[i].pdf = sc.pdf; out[i].flags = (sc.delta ? 1u : 0u) | (sc.medium ? 2u : 0u);
  }
}
void host_face_mat_eval_n(const void *image, const CrtMaterial *mats, size_t n_mats, const CrtShadeQuery *qs, const CrtFaceCoord *coords,
                          size_t n, CrtBsdfEval *out) {
  const FaceView F = view(image);
  for (size_t i = 0; i < n; i++) {
    std::memset(&out[i], 0, sizeof out[i]);
    if (qs[i].material >= n_mats) continue;
    const CrtMaterial &m = mats[qs[i].material];
    const MatFace mv{m, BaseTexel{base_of(F, m, qs[i].material, coords[i])}};
    V3 value; float pdf;
    if (!mat_eval<false, MatFace>(mv, v3(qs[i].ray_dir[0], qs[i].ray_dir[1], qs[i].ray_dir[2]), rec_of(qs[i]),
                                  v3(qs[i].wi[0], qs[i].wi[1], qs[i].wi[2]), value, pdf)) continue;
    put(out[i].value, value); out[i].pdf = pdf; out[i].some = 1;
  }
}

}  // extern "C"
