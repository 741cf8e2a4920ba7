/* libcrt_amd: per-face (Ptex-style) colour textures — the decoded atlas, the face maps that survive triangulation and the
 * bindings that tie them to geometries and materials, as one aggregate with batched device functions. A header of its
 * own beside crt.h, as crt_render_volumes.h and crt_guiding.h are: crt.h's set of declarations stays as it is. Exported
 * by the same library; include it after, or instead of, crt.h.
 *
 * What the reference keeps in four places is one object here:
 *  - textures:  `PtexTexture` as the renderer's host decodes it (crust-render main.rs:172-319): per face a rectangle of
 *               linear RGB texels, row-major within the face, v-major, sampled bilinearly with clamped borders; a
 *               fallback colour for a face that does not exist or has no texels (the reference uses 0.5 grey).
 *  - face maps: `FaceMap` (rt_world.rs:20-78): per triangle of a mesh the source polygon and the slice of its fan.
 *  - bindings:  `World::faces` / `set_face_map`: top-level geom_id -> (map, swapped). For an instance the key is the
 *               instance's id while prim_id stays the inner mesh's, as a hit reports them.
 *  - material bindings: `base_color_ptex`: material index -> texture index, or CRT_INVALID_ID.
 * Decoding .ptx files is the host's business (the reference keeps it behind its AssetLoader seam too), and so is
 * filtering across faces, which the reference does not attempt either.
 *
 * Limits: a face is at most 16384 x 16384 texels (CRUST_PTEX_MAX_LOG2 <= 14); a binding's geom_id is below
 * CRT_FACE_MAX_GEOMS; the device image — texels stored as 16 bytes each, plus the tables — is below 4 GiB.
 *
 * emitted_directional keeps the authored colour, as upstream (openpbr.rs:1211-1218): there is no textured form of
 * crt_material_emitted_n. */
#ifndef CRT_FACE_TEXTURES_H
#define CRT_FACE_TEXTURES_H

#include "crt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_NO_FACE 0xFFFFFFFFu /* HitRecord::NO_FACE */
#define CRT_FACE_MAX_RES 16384u
#define CRT_FACE_MAX_GEOMS (1u << 24)

/* FanSlice (rt_world.rs:20-32): which triangle of a polygon's fan a primitive is. */
enum CrtFanSlice { CRT_FAN_TRIANGLE = 0, CRT_FAN_QUAD_LOWER = 1, CRT_FAN_QUAD_UPPER = 2, CRT_FAN_UNMAPPABLE = 3 };

/* One face's texels within its texture (main.rs:173-177). offset counts texels (RGB triples), not floats: the face's
 * texel (x, y) is texels[3 * (offset + y * width + x) ..][0..3]. 8 bytes. width or height 0 is legal: the face answers
 * the fallback (main.rs:282). */
typedef struct CrtFaceRect {
  uint32_t offset;
  uint16_t width, height;
} CrtFaceRect;

typedef struct CrtFaceTexture {
  const CrtFaceRect *faces; /* [n_faces] */
  size_t n_faces;
  const float *texels;      /* [3 * n_texels] linear RGB */
  size_t n_texels;
  float fallback[3];
} CrtFaceTexture;

typedef struct CrtFaceMap {
  const uint32_t *faces;    /* [n_prims] source polygon (the texture's face id) per triangle, indexed by prim_id */
  const uint8_t *slices;    /* [n_prims] CrtFanSlice */
  size_t n_prims;
} CrtFaceMap;

/* 12 bytes. swapped != 0: the placement baked a mirrored winding, u and v trade places before the slice is applied. */
typedef struct CrtFaceBinding {
  uint32_t geom_id, map, swapped;
} CrtFaceBinding;

/* What crt_face_resolve_n writes and the textured calls read. 16 bytes. face_id == CRT_NO_FACE: no face, u = v = 0. */
typedef struct CrtFaceCoord {
  uint32_t face_id;
  float u, v;
  uint32_t _pad;
} CrtFaceCoord;

/* The head of the image the kernels read (crt_face_textures_image); every off_* is in bytes from the image's start.
 *   textures  n_textures x { u32 first_face, n_faces; f32 fallback[3]; u32 pad[3] }                       (32 bytes)
 *   faces     n_faces_total x { u32 texel (index into the texel plane), u16 width, height }               (8 bytes)
 *   maps      n_maps x { u32 first_prim, n_prims, pad[2] }                                               (16 bytes)
 *   map_faces / map_slices   n_prims_total x u32 / x u8
 *   geoms     n_geoms x u32: map | swapped << 31, or CRT_INVALID_ID for a geometry without a binding
 *   material_texture  n_materials x u32
 *   texels    n_texels_total x { f32 r, g, b, 0 }                                                         (16 bytes)
 * Every table starts on a 256-byte boundary. 68 bytes. */
typedef struct CrtFaceTexturesHeader {
  uint32_t magic, bytes;
  uint32_t n_textures, n_faces_total, n_maps, n_prims_total, n_geoms, n_materials, n_texels_total;
  uint32_t off_textures, off_faces, off_maps, off_map_faces, off_map_slices, off_geoms, off_material_texture, off_texels;
} CrtFaceTexturesHeader;

typedef struct CrtFaceTextures CrtFaceTextures;

/* Builds the aggregate; every array is copied. Touches no device: the image is uploaded on first device use. NULL with the
 * reason in crt_last_error: a NULL array with a non-zero count; a binding that names a map, or a material binding that
 * names a texture, which does not exist; two bindings of one geom_id; a geom_id at or above CRT_FACE_MAX_GEOMS; a face
 * wider or taller than CRT_FACE_MAX_RES, or one whose texels run past n_texels; a slice value above
 * CRT_FAN_UNMAPPABLE; a texel or a fallback that is not finite; an image of 4 GiB or more. */
CrtFaceTextures *crt_face_textures_new(const CrtFaceTexture *textures, size_t n_textures, const CrtFaceMap *maps, size_t n_maps,
                                       const CrtFaceBinding *bindings, size_t n_bindings, const uint32_t *material_texture,
                                       size_t n_materials);
/* Drops the caller's reference. */
void crt_face_textures_free(CrtFaceTextures *ft);
/* The image the kernels read, in host memory, valid while the handle lives (for tests and tools). */
int crt_face_textures_image(const CrtFaceTextures *ft, const void **image, size_t *bytes);

/* The batched entry points take device pointers and a stream and do not synchronise, like the shading seam of crt.h.
 * n == 0 is CRT_OK and launches nothing.
 * One aggregate serves ONE device: its image is uploaded to the device that is current at the first of these calls, and
 * every later call must be made with that device current (CRT_ERR_UNSUPPORTED otherwise, the reason in crt_last_error); a
 * host that drives several GPUs builds one aggregate per device. crt_face_textures_free releases the image on its own
 * device whichever is current.
 *
 * World::intersect's face lookup (rt_world.rs:207-232) for hits as crt_intersect_n wrote them: the binding of the hit's
 * geom_id, FaceMap::resolve (rt_world.rs:64-77: the swap, then QuadLower (u + v, v), QuadUpper (u, u + v), Triangle
 * (u, v), both clamped to [0, 1]). CRT_NO_FACE and (0, 0) for a miss, a geometry without a binding, a prim_id past the
 * map and an Unmappable slice. */
int crt_face_resolve_n(CrtFaceTextures *ft, const CrtRayHit *d_hits, size_t n, CrtFaceCoord *d_coords, void *stream);
/* PtexTexture::eval (main.rs:277-314) of texture `texture` at every coordinate: d_rgb takes 3 floats per query. A face id
 * past the texture's faces (CRT_NO_FACE included) and a face without texels answer the fallback; a coordinate that is
 * not finite reads as 0. CRT_ERR_BAD_ARG when `texture` names none. */
int crt_face_texture_eval_n(CrtFaceTextures *ft, uint32_t texture, const CrtFaceCoord *d_coords, size_t n, float *d_rgb, void *stream);
/* crt_material_scatter_n / crt_material_eval_n (crt.h) with OpenPBR::shaded's substitution (openpbr.rs:1011-1024,
 * :1162-1180): where material_texture[query.material] names a texture and d_coords[i].face_id != CRT_NO_FACE, the call
 * runs on that material with base_color replaced by the texture's value at the coordinate — before the lobe pmf is
 * built, so lobe selection follows the texture. Every other query is exactly the untextured call. d_coords is
 * index-parallel with d_queries. */
int crt_material_scatter_faces_n(CrtFaceTextures *ft, const CrtMaterial *d_materials, size_t n_materials, const CrtShadeQuery *d_queries,
                                 const CrtFaceCoord *d_coords, size_t n, CrtScatterSample *d_out, void *stream);
int crt_material_eval_faces_n(CrtFaceTextures *ft, const CrtMaterial *d_materials, size_t n_materials, const CrtShadeQuery *d_queries,
                              const CrtFaceCoord *d_coords, size_t n, CrtBsdfEval *d_out, void *stream);

/* Binds the aggregate to a wavefront renderer (World::faces and base_color_ptex of the world the renderer draws), or
 * detaches it (ft == NULL). The renderer keeps a reference of its own; the image is uploaded inside the call; the call
 * waits for the renderer's batches in flight; the binding holds from the next crt_render_samples on. A bound renderer runs
 * one launch per stage whatever the batch size: the extend instance also keeps (prim_id, u, v) of every hit, and the
 * shade instances resolve the face of a hit on a bound geometry, sample the texture of its material — material_texture
 * is indexed by the hit's geom_id, as the renderer's material table is — and run scatter and both evals of the vertex
 * with the texel in the place of base_color. A hit without a binding, without a texture or without a face shades with
 * the authored colour, to the bits of the unbound renderer; emission keeps the authored colour. crt_renderer_pipeline
 * reports the form as | 512 in out[1]. CRT_ERR_BAD_ARG: r == NULL, or a binding whose geom_id or material index is past
 * the renderer's tables; CRT_ERR_NO_DEVICE: the upload failed; CRT_ERR_UNSUPPORTED (the text in crt_last_error): a volume
 * aggregate is bound — crt_renderer_set_volumes answers the same while this one is — or the build is a CRT_REGEN_FIRST
 * build. crt_render_samples_stats answers CRT_ERR_UNSUPPORTED while an aggregate is bound. */
int crt_renderer_set_face_textures(CrtRenderer *r, CrtFaceTextures *ft);

#ifdef __cplusplus
}
#endif

#endif
