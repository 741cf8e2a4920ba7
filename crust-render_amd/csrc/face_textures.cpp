// The per-face texture aggregate on the host: the checks of crt_face_textures_new, the image the kernels read
// (include/crt_face_textures.h: CrtFaceTexturesHeader; kernels/faces.hip.h: the records) and the handle's life. Building
// touches no device: the image is uploaded on first device use.
//
// What the image changes about the inputs: a face's texel offset becomes absolute (its texture's first texel added), a
// texel grows a fourth float of 0, and the bindings become one word per geometry, 0 .. the largest bound geom_id.
#include <algorithm>
#include <cstring>
#include <new>
#include <utility>

#include "crt_internal.h"
#include "face_textures_internal.h"
#include "kernels/faces.hip.h"

namespace crt {

using dev::FaceMapRec;
using dev::FaceRectRec;
using dev::FaceTexRec;
using dev::FaceView;

int face_textures_build_image(const CrtFaceTexture *textures, size_t n_textures, const CrtFaceMap *maps, size_t n_maps,
                              const CrtFaceBinding *bindings, size_t n_bindings, const uint32_t *material_texture, size_t n_materials,
                              std::vector<unsigned char> &image) {
  const char *who = "crt_face_textures_new";
  if ((n_textures && !textures) || (n_maps && !maps) || (n_bindings && !bindings) || (n_materials && !material_texture)) {
    set_error_text("%s: a NULL array with a non-zero count", who);
    return CRT_ERR_BAD_ARG;
  }
  const uint64_t kLimit = 0xffffffffull;  // the image's byte size and every count in it are 32-bit
  if (n_textures > kLimit || n_maps > 0x7fffffffull || n_bindings > kLimit || n_materials > kLimit) {
    set_error_text("%s: a table of more than 2^32 entries", who);
    return CRT_ERR_BAD_ARG;
  }
  uint64_t faces_total = 0, texels_total = 0, prims_total = 0;
  for (size_t t = 0; t < n_textures; t++) {
    const CrtFaceTexture &T = textures[t];
    if ((T.n_faces && !T.faces) || (T.n_texels && !T.texels)) {
      set_error_text("%s: texture %zu has a NULL array with a non-zero count", who, t);
      return CRT_ERR_BAD_ARG;
    }
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(T.fallback[c])) { set_error_text("%s: texture %zu has a fallback colour that is not finite", who, t); return CRT_ERR_BAD_ARG; }
    for (size_t f = 0; f < T.n_faces; f++) {
      const CrtFaceRect &R = T.faces[f];
      if (R.width > CRT_FACE_MAX_RES || R.height > CRT_FACE_MAX_RES) {
        set_error_text("%s: face %zu of texture %zu is %u x %u texels (at most %u either way)", who, f, t, (unsigned)R.width,
                       (unsigned)R.height, CRT_FACE_MAX_RES);
        return CRT_ERR_BAD_ARG;
      }
      const uint64_t end = (uint64_t)R.offset + (uint64_t)R.width * R.height;
      if (end > T.n_texels) {
        set_error_text("%s: face %zu of texture %zu reads texels %u .. %llu of %zu", who, f, t, R.offset, (unsigned long long)end, T.n_texels);
        return CRT_ERR_BAD_ARG;
      }
    }
    faces_total += T.n_faces;
    texels_total += T.n_texels;
    if (faces_total > kLimit || texels_total > kLimit / 16) {
      set_error_text("%s: the device image would reach 4 GiB (%llu texels, %llu faces by texture %zu)", who,
                     (unsigned long long)texels_total, (unsigned long long)faces_total, t);
      return CRT_ERR_BAD_ARG;
    }
    for (size_t i = 0; i < 3 * T.n_texels; i++)
      if (!std::isfinite(T.texels[i])) {
        set_error_text("%s: texel %zu of texture %zu has a channel that is not finite", who, i / 3, t);
        return CRT_ERR_BAD_ARG;
      }
  }
  for (size_t m = 0; m < n_maps; m++) {
    const CrtFaceMap &M = maps[m];
    if (M.n_prims && (!M.faces || !M.slices)) { set_error_text("%s: map %zu has a NULL array with a non-zero count", who, m); return CRT_ERR_BAD_ARG; }
    for (size_t p = 0; p < M.n_prims; p++)
      if (M.slices[p] > CRT_FAN_UNMAPPABLE) {
        set_error_text("%s: primitive %zu of map %zu has the unknown slice %u", who, p, m, (unsigned)M.slices[p]);
        return CRT_ERR_BAD_ARG;
      }
    prims_total += M.n_prims;
    if (prims_total > kLimit / 8) {
      set_error_text("%s: the device image would reach 4 GiB (%llu primitives by map %zu)", who, (unsigned long long)prims_total, m);
      return CRT_ERR_BAD_ARG;
    }
  }
  uint32_t n_geoms = 0;
  for (size_t b = 0; b < n_bindings; b++) {
    if (bindings[b].geom_id >= CRT_FACE_MAX_GEOMS) {
      set_error_text("%s: binding %zu names geometry %u (below %u)", who, b, bindings[b].geom_id, CRT_FACE_MAX_GEOMS);
      return CRT_ERR_BAD_ARG;
    }
    if (bindings[b].map >= n_maps) {
      set_error_text("%s: binding %zu names map %u of %zu", who, b, bindings[b].map, n_maps);
      return CRT_ERR_BAD_ARG;
    }
    if (bindings[b].geom_id + 1 > n_geoms) n_geoms = bindings[b].geom_id + 1;
  }
  {  // a geometry bound twice: found here, over the bindings alone, before anything of the image exists
    std::vector<std::pair<uint32_t, size_t>> by_geom(n_bindings);
    for (size_t b = 0; b < n_bindings; b++) by_geom[b] = {bindings[b].geom_id, b};
    std::sort(by_geom.begin(), by_geom.end());
    size_t dup = n_bindings;  // the earliest binding that repeats a geometry
    for (size_t k = 1; k < n_bindings; k++)
      if (by_geom[k].first == by_geom[k - 1].first && by_geom[k].second < dup) dup = by_geom[k].second;
    if (dup != n_bindings) {
      set_error_text("%s: binding %zu names geometry %u, which is bound already", who, dup, bindings[dup].geom_id);
      return CRT_ERR_BAD_ARG;
    }
  }
  for (size_t m = 0; m < n_materials; m++)
    if (material_texture[m] != CRT_INVALID_ID && material_texture[m] >= n_textures) {
      set_error_text("%s: material %zu names texture %u of %zu", who, m, material_texture[m], n_textures);
      return CRT_ERR_BAD_ARG;
    }

  auto up = [](uint64_t v) { return (v + 255) & ~(uint64_t)255; };
  CrtFaceTexturesHeader hd;
  std::memset(&hd, 0, sizeof(hd));
  uint64_t at = up(sizeof(hd));
  auto place = [&](uint64_t bytes) { const uint64_t o = at; at = up(at + bytes); return o; };
  const uint64_t o_tex = place(n_textures * sizeof(FaceTexRec)), o_faces = place(faces_total * sizeof(FaceRectRec));
  const uint64_t o_maps = place(n_maps * sizeof(FaceMapRec)), o_mf = place(prims_total * 4), o_ms = place(prims_total);
  const uint64_t o_geoms = place((uint64_t)n_geoms * 4), o_mt = place(n_materials * 4);
  const uint64_t o_texels = place(texels_total * 16 + 16);  // never empty: the kernels are handed a texel pointer
  if (at > kLimit) { set_error_text("%s: the device image would be %llu bytes (below 4 GiB)", who, (unsigned long long)at); return CRT_ERR_BAD_ARG; }
  hd.magic = dev::kFaceMagic; hd.bytes = (uint32_t)at;
  hd.n_textures = (uint32_t)n_textures; hd.n_faces_total = (uint32_t)faces_total; hd.n_maps = (uint32_t)n_maps;
  hd.n_prims_total = (uint32_t)prims_total; hd.n_geoms = n_geoms; hd.n_materials = (uint32_t)n_materials;
  hd.n_texels_total = (uint32_t)texels_total;
  hd.off_textures = (uint32_t)o_tex; hd.off_faces = (uint32_t)o_faces; hd.off_maps = (uint32_t)o_maps; hd.off_map_faces = (uint32_t)o_mf;
  hd.off_map_slices = (uint32_t)o_ms; hd.off_geoms = (uint32_t)o_geoms; hd.off_material_texture = (uint32_t)o_mt; hd.off_texels = (uint32_t)o_texels;
  image.assign((size_t)at, 0);
  unsigned char *im = image.data();
  std::memcpy(im, &hd, sizeof(hd));
  FaceTexRec *tex = reinterpret_cast<FaceTexRec *>(im + o_tex);
  FaceRectRec *rect = reinterpret_cast<FaceRectRec *>(im + o_faces);
  float *texel = reinterpret_cast<float *>(im + o_texels);
  uint32_t face_at = 0, texel_at = 0;
  for (size_t t = 0; t < n_textures; t++) {
    const CrtFaceTexture &T = textures[t];
    tex[t].first_face = face_at; tex[t].n_faces = (uint32_t)T.n_faces;
    for (int c = 0; c < 3; c++) tex[t].fallback[c] = T.fallback[c];
    for (size_t f = 0; f < T.n_faces; f++) rect[face_at + f] = FaceRectRec{texel_at + T.faces[f].offset, T.faces[f].width, T.faces[f].height};
    for (size_t i = 0; i < T.n_texels; i++) {
      float *o = texel + 4 * ((size_t)texel_at + i);
      o[0] = T.texels[3 * i]; o[1] = T.texels[3 * i + 1]; o[2] = T.texels[3 * i + 2];
    }
    face_at += (uint32_t)T.n_faces; texel_at += (uint32_t)T.n_texels;
  }
  FaceMapRec *map = reinterpret_cast<FaceMapRec *>(im + o_maps);
  uint32_t prim_at = 0;
  for (size_t m = 0; m < n_maps; m++) {
    map[m].first_prim = prim_at; map[m].n_prims = (uint32_t)maps[m].n_prims;
    if (maps[m].n_prims) {
      std::memcpy(im + o_mf + 4 * (size_t)prim_at, maps[m].faces, 4 * maps[m].n_prims);
      std::memcpy(im + o_ms + prim_at, maps[m].slices, maps[m].n_prims);
    }
    prim_at += (uint32_t)maps[m].n_prims;
  }
  uint32_t *geoms = reinterpret_cast<uint32_t *>(im + o_geoms);
  for (uint32_t g = 0; g < n_geoms; g++) geoms[g] = dev::kFaceNone;
  for (size_t b = 0; b < n_bindings; b++) geoms[bindings[b].geom_id] = bindings[b].map | (bindings[b].swapped ? 0x80000000u : 0u);
  if (n_materials) std::memcpy(im + o_mt, material_texture, 4 * n_materials);
  return CRT_OK;
}

void face_view_of(const unsigned char *host_image, const unsigned char *base, FaceView &out) {
  const CrtFaceTexturesHeader *hd = reinterpret_cast<const CrtFaceTexturesHeader *>(host_image);
  out.textures = reinterpret_cast<const FaceTexRec *>(base + hd->off_textures);
  out.faces = reinterpret_cast<const FaceRectRec *>(base + hd->off_faces);
  out.maps = reinterpret_cast<const FaceMapRec *>(base + hd->off_maps);
  out.map_faces = reinterpret_cast<const uint32_t *>(base + hd->off_map_faces);
  out.map_slices = base + hd->off_map_slices;
  out.geoms = reinterpret_cast<const uint32_t *>(base + hd->off_geoms);
  out.material_texture = reinterpret_cast<const uint32_t *>(base + hd->off_material_texture);
  out.texels = reinterpret_cast<const float4 *>(base + hd->off_texels);
  out.n_textures = hd->n_textures; out.n_maps = hd->n_maps; out.n_geoms = hd->n_geoms; out.n_materials = hd->n_materials;
}

}  // namespace crt

// Everything above is plain host C++: the stand-alone sanitizer program (profiles/host_shade/face_textures_sanitize.cpp)
// compiles it without the rest of the library.
#ifndef CRT_FACE_TEXTURES_BUILDER_ONLY

namespace crt {

struct FaceTextures {
  std::vector<unsigned char> image;
  std::mutex mu;
  void *d_image = nullptr;  // uploaded on first device use, to the device current then
  int device = -1;          // ... which is the one device this aggregate serves (crt_face_textures.h)
  ~FaceTextures() {
    if (d_image) {
      int cur = -1;  // synchronise and free on the image's own device, whatever is current here
      const bool moved = hipGetDevice(&cur) == hipSuccess && cur != device && hipSetDevice(device) == hipSuccess;
      (void)hipDeviceSynchronize();  // nothing that was handed the image may still be reading it
      (void)hipFree(d_image);
      if (moved) (void)hipSetDevice(cur);
    }
  }
};

}  // namespace crt

struct CrtFaceTextures { std::shared_ptr<crt::FaceTextures> p; std::atomic<int> refs{1}; };

namespace crt {

int face_textures_device(CrtFaceTextures *ft, FaceView &out) {
  FaceTextures &T = *ft->p;
  std::lock_guard<std::mutex> lock(T.mu);
  int cur = -1;
  if (!T.d_image) {
    if (!device_ok()) return CRT_ERR_NO_DEVICE;
    if (!CRT_HIP_OK(hipGetDevice(&cur))) return CRT_ERR_NO_DEVICE;
    void *d = nullptr;
    if (!CRT_HIP_OK(hipMalloc(&d, T.image.size()))) return CRT_ERR_NO_DEVICE;
    if (!CRT_HIP_OK(hipMemcpy(d, T.image.data(), T.image.size(), hipMemcpyHostToDevice))) { (void)hipFree(d); return CRT_ERR_NO_DEVICE; }
    T.d_image = d;
    T.device = cur;
  } else {
    if (!CRT_HIP_OK(hipGetDevice(&cur))) return CRT_ERR_NO_DEVICE;
    if (cur != T.device) {  // a pointer into device A's memory must not reach a launch on device B
      set_error_text("crt_face_textures: the aggregate's image lives on device %d and the current device is %d", T.device, cur);
      return CRT_ERR_UNSUPPORTED;
    }
  }
  face_view_of(T.image.data(), static_cast<const unsigned char *>(T.d_image), out);
  return CRT_OK;
}

uint32_t face_textures_texture_count(const CrtFaceTextures *ft) {
  return reinterpret_cast<const CrtFaceTexturesHeader *>(ft->p->image.data())->n_textures;
}

void face_textures_counts(const CrtFaceTextures *ft, uint32_t &n_geoms, uint32_t &n_materials) {
  const CrtFaceTexturesHeader *hd = reinterpret_cast<const CrtFaceTexturesHeader *>(ft->p->image.data());
  n_geoms = hd->n_geoms; n_materials = hd->n_materials;
}

void face_textures_retain(CrtFaceTextures *ft) { if (ft) ft->refs.fetch_add(1, std::memory_order_relaxed); }
void face_textures_release(CrtFaceTextures *ft) { if (ft && ft->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete ft; }

}  // namespace crt

using namespace crt;

extern "C" {

CrtFaceTextures *crt_face_textures_new(const CrtFaceTexture *textures, size_t n_textures, const CrtFaceMap *maps, size_t n_maps,
                                       const CrtFaceBinding *bindings, size_t n_bindings, const uint32_t *material_texture,
                                       size_t n_materials) {
  CrtFaceTextures *out = nullptr;
  (void)abi_guard("crt_face_textures_new", [&] {
    auto t = std::make_shared<FaceTextures>();
    const int rc = face_textures_build_image(textures, n_textures, maps, n_maps, bindings, n_bindings, material_texture, n_materials, t->image);
    if (rc != CRT_OK) return rc;
    CrtFaceTextures *handle = new CrtFaceTextures();
    handle->p = std::move(t);
    out = handle;
    return (int)CRT_OK;
  });
  return out;
}

void crt_face_textures_free(CrtFaceTextures *ft) { face_textures_release(ft); }

int crt_face_textures_image(const CrtFaceTextures *ft, const void **image, size_t *bytes) {
  if (!ft || !image || !bytes) return CRT_ERR_BAD_ARG;
  *image = ft->p->image.data();
  *bytes = ft->p->image.size();
  return CRT_OK;
}

}  // extern "C"

#endif  // CRT_FACE_TEXTURES_BUILDER_ONLY
