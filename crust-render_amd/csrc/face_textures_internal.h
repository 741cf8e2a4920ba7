// Per-face textures inside the library (face_textures.cpp, kernels/faces_seam.hip): the image builder and the device
// view of a handle. Kept out of crt_internal.h, as guiding_internal.h is: only these two files need it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/crt_face_textures.h"

namespace crt {

namespace dev { struct FaceView; }

// CRT_OK and the image (include/crt_face_textures.h: CrtFaceTexturesHeader), or CRT_ERR_BAD_ARG with the reason in
// crt_last_error. Plain host C++, no device.
int face_textures_build_image(const CrtFaceTexture *textures, size_t n_textures, const CrtFaceMap *maps, size_t n_maps,
                              const CrtFaceBinding *bindings, size_t n_bindings, const uint32_t *material_texture, size_t n_materials,
                              std::vector<unsigned char> &image);
// The tables of an image at `base` (the host image, or its device copy) as the kernels take them.
void face_view_of(const unsigned char *host_image, const unsigned char *base, dev::FaceView &out);
// The device copy of a handle's image (uploaded on first use).
int face_textures_device(CrtFaceTextures *ft, dev::FaceView &out);
uint32_t face_textures_texture_count(const CrtFaceTextures *ft);
// The geometry and material tables' lengths: every binding names an index below them.
void face_textures_counts(const CrtFaceTextures *ft, uint32_t &n_geoms, uint32_t &n_materials);
// A handle is reference counted: crt_face_textures_new hands the caller one reference, crt_face_textures_free drops it.
void face_textures_retain(CrtFaceTextures *ft);
void face_textures_release(CrtFaceTextures *ft);

}  // namespace crt
