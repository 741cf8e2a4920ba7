// Per-face colour textures on the device: FaceMap::resolve (rt_world.rs:64-77) behind World::intersect's binding lookup
// (rt_world.rs:207-232), and PtexTexture::eval as the reference's host implements it (crust-render main.rs:277-314),
// operation for operation. Written once: the seam kernels (faces_seam.hip) and the host-compiled twin of the tests
// (tests/host_shade/faces_host.cpp) include this file. The image is the one face_textures.cpp builds
// (include/crt_face_textures.h: CrtFaceTexturesHeader); a texel is 16 bytes so that a corner is one load, and its fourth
// float never enters arithmetic.
// Compile with -ffp-contract=off (dmath.hip.h).
#pragma once

#include "dmath.hip.h"

namespace crt {
namespace dev {

constexpr uint32_t kFaceMagic = 0x58545046u;  // "FPTX"
constexpr uint32_t kNoFace = 0xFFFFFFFFu;     // CRT_NO_FACE
constexpr uint32_t kFaceNone = 0xFFFFFFFFu;   // CRT_INVALID_ID in the geometry and material tables
enum { kFanTriangle = 0, kFanQuadLower = 1, kFanQuadUpper = 2, kFanUnmappable = 3 };

struct FaceTexRec { uint32_t first_face, n_faces; float fallback[3]; uint32_t pad[3]; };
struct FaceRectRec { uint32_t texel; uint16_t width, height; };
struct FaceMapRec { uint32_t first_prim, n_prims, pad[2]; };
static_assert(sizeof(FaceTexRec) == 32 && sizeof(FaceRectRec) == 8 && sizeof(FaceMapRec) == 16, "crt_face_textures.h image records");

// The image's tables as the kernels take them (pointers into the device copy; into the host image in the tests).
struct FaceView {
  const FaceTexRec *textures;
  const FaceRectRec *faces;
  const FaceMapRec *maps;
  const uint32_t *map_faces;
  const uint8_t *map_slices;
  const uint32_t *geoms;
  const uint32_t *material_texture;
  const float4 *texels;
  uint32_t n_textures, n_maps, n_geoms, n_materials;
};

struct FaceCoord { uint32_t face; float u, v; };

// World::intersect's lookup: the geometry's binding, then FaceMap::resolve. `None` is {kNoFace, 0, 0}.
__device__ __forceinline__ FaceCoord face_resolve(const FaceView &F, uint32_t geom_id, uint32_t prim, float u, float v) {
  const FaceCoord none{kNoFace, 0.0f, 0.0f};
  if (geom_id >= F.n_geoms) return none;
  const uint32_t b = F.geoms[geom_id];
  if (b == kFaceNone) return none;
  const FaceMapRec m = F.maps[b & 0x7fffffffu];
  if (prim >= m.n_prims) return none;
  const uint32_t face = F.map_faces[m.first_prim + prim];
  const uint32_t slice = F.map_slices[m.first_prim + prim];
  if (b >> 31) { const float t = u; u = v; v = t; }
  float fu, fv;
  if (slice == kFanQuadLower) { fu = u + v; fv = v; }
  else if (slice == kFanQuadUpper) { fu = u; fv = u + v; }
  else if (slice == kFanTriangle) { fu = u; fv = v; }
  else return none;
  return FaceCoord{face, rclamp(fu, 0.0f, 1.0f), rclamp(fv, 0.0f, 1.0f)};
}

__device__ __forceinline__ bool face_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
// (c.max(0.0) as usize).min(n - 1); c is a whole number in [-1, n]
__device__ __forceinline__ uint32_t face_index(float c, uint32_t n) {
  const uint32_t i = (uint32_t)rmax(c, 0.0f);
  return i < n - 1 ? i : n - 1;
}
__device__ __forceinline__ V3 face_texel(const float4 *texels, uint32_t base, uint32_t w, uint32_t x, uint32_t y) {
  const float4 t = texels[base + (y * w + x)];
  return v3(t.x, t.y, t.z);
}

// PtexTexture::eval: bilinear, borders clamped, texel centres at (i + 0.5) / n. tex < F.n_textures is the caller's.
__device__ __forceinline__ V3 face_texture_eval(const FaceView &F, uint32_t tex, uint32_t face, float u, float v) {
  const FaceTexRec &T = F.textures[tex];
  const V3 fallback = v3(T.fallback[0], T.fallback[1], T.fallback[2]);
  if (face >= T.n_faces) return fallback;
  const FaceRectRec f = F.faces[T.first_face + face];
  const uint32_t w = f.width, h = f.height;
  if (w == 0 || h == 0) return fallback;
  const float fu = face_finite(u) ? rclamp(u, 0.0f, 1.0f) : 0.0f;
  const float fv = face_finite(v) ? rclamp(v, 0.0f, 1.0f) : 0.0f;
  const float x = fu * (float)w - 0.5f;
  const float y = fv * (float)h - 0.5f;
  const float x0 = floorf(x);
  const float y0 = floorf(y);
  const float tx = x - x0;
  const float ty = y - y0;
  const uint32_t x0i = face_index(x0, w), x1i = face_index(x0 + 1.0f, w);
  const uint32_t y0i = face_index(y0, h), y1i = face_index(y0 + 1.0f, h);
  const V3 top = lerp(face_texel(F.texels, f.texel, w, x0i, y0i), face_texel(F.texels, f.texel, w, x1i, y0i), tx);
  const V3 bot = lerp(face_texel(F.texels, f.texel, w, x0i, y1i), face_texel(F.texels, f.texel, w, x1i, y1i), tx);
  return lerp(top, bot, ty);
}

}  // namespace dev
}  // namespace crt
