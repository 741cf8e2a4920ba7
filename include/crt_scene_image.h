/* libcrt_amd: the scene image on the host — the one entry point that hands out the arrays Scene::ensure_device would
 * upload. A header of its own beside crt.h: crt.h's set of declarations is pinned as it stood when the volume aggregate
 * went behind the ABI (tests/test_volumes.py), and this entry point came after. Exported by the same library; include it
 * after, or instead of, crt.h. */
#ifndef CRT_SCENE_IMAGE_H
#define CRT_SCENE_IMAGE_H

#include "crt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only (no GPU needed): one array of the image crt_scene_image_check verifies, as bytes, in the layout the kernels
 * read — which: 0 nodes (128 bytes each), 1 leaf records (16), 2 Tri4 packets (192), 3 the leaves' index lists (4), 4
 * primitive records (64), 5 instance records (64), 6 shading normals and moving placements (floats) — and the image's
 * plain fields in view: root node (CRT_INVALID_ID: an empty scene), whether the queried tree has packets, node count,
 * packet count, 1 if direct leaf words occur, LDS stack split, cold-state bits, 0. n_bytes receives the array's size; at
 * most cap_bytes are copied to dst (which may be NULL when cap_bytes is 0). A host build of a traversal header runs on
 * these arrays (tests/test_camera_trace_host.py: kernels/traverse_camera.hip.h against the oracle). CRT_ERR_BAD_ARG: a
 * NULL argument, or which > 6. */
int crt_scene_image_array(CrtScene *s, uint32_t which, void *dst, size_t cap_bytes, size_t *n_bytes, uint32_t view[8]);

#ifdef __cplusplus
}
#endif

#endif
