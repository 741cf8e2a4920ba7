// Internal host/device declarations of libcrt_amd.so (not part of the ABI).
//
// Host side (C++17): geometry table, deterministic SBVH -> BVH4 build, flattening of a committed
// scene and everything it instances into ONE device image with absolute indices.
// Device side (HIP, gfx950): see kernels/.
// The device image format the two sides share is dev_image.h; which engine and which kernel instances run is
// launch_plan.h. Both are included here, so the host sources see everything through this one header.
#pragma once

#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/crt.h"
#include "../../include/crt_render_volumes.h"
#include "../../include/crt_scene_image.h"
#include "dev_image.h"
#include "launch_plan.h"

namespace crt {

// ---------------------------------------------------------------------------------------------
// Small float3 with glam Vec3A (SSE2) semantics. Compiled -ffp-contract=off.
// ---------------------------------------------------------------------------------------------
struct F3 {
  float x, y, z;
  float operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
  float &at(int i) { return i == 0 ? x : (i == 1 ? y : z); }
};
inline F3 f3(float x, float y, float z) { return F3{x, y, z}; }
inline F3 operator+(F3 a, F3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline F3 operator-(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline F3 operator*(F3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline F3 operator-(F3 a) { return {-a.x, -a.y, -a.z}; }
inline float sse_min(float a, float b) { return a < b ? a : b; }  // minps
inline float sse_max(float a, float b) { return a > b ? a : b; }  // maxps
inline F3 vmin(F3 a, F3 b) { return {sse_min(a.x, b.x), sse_min(a.y, b.y), sse_min(a.z, b.z)}; }
inline F3 vmax(F3 a, F3 b) { return {sse_max(a.x, b.x), sse_max(a.y, b.y), sse_max(a.z, b.z)}; }
inline float dot(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline F3 cross(F3 a, F3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }

struct Aabb { F3 mn, mx; };
struct Affine { F3 x, y, z, t; };  // glam Affine3A: matrix3 columns + translation
struct Mat3 { F3 x, y, z; };

Affine affine_inverse(const Affine &a);
Mat3 mat3_transpose(const Mat3 &m);
F3 affine_point(const Affine &a, F3 p);
F3 affine_vector(const Affine &a, F3 p);
Aabb transformed_aabb(const Aabb &local, const Affine &m);  // prim.rs:298-319

struct Scene;

// Host primitive (prim.rs:60-70, :125-130, :261-280).
struct Prim {
  PrimKind kind;
  uint32_t geom_id, prim_id, mask;
  F3 v0, v1, v2;
  bool has_normals;
  F3 n0, n1, n2;
  F3 center;
  float radius;
  float radius1;  // PRIM_CURVE (prim.rs:175-183): p0 = v0, p1 = v1, r0 = radius, r1 = radius1
  F3 v3;          // PRIM_CUBIC (prim.rs:220-227): cp = v0 v1 v2 v3, r0 = radius, r1 = radius1
  uint32_t depth; // PRIM_CUBIC: cubic_flatness_depth of the span, computed once at commit
  std::shared_ptr<Scene> scene;
  Affine l2w, w2l;
  Mat3 normal_mat;
  bool has_end;
  Affine l2w_end;
  Aabb bounds;
};

struct Bvh {
  std::vector<WideNode> wide;
  std::vector<Leaf> leaves;
  std::vector<Tri4> packets;
  std::vector<uint32_t> indices;
  std::vector<Prim> prims;
  bool has_bbox = false;
  Aabb root_bbox{};
};

// Instance nesting the traversal kernels carry frames for (kernels/traverse.hip.h kMaxLevels; the importer's own
// limit, usd_import.rs:60 MAX_INSTANCE_NESTING): commit refuses deeper scenes instead of skipping instances at trace time.
constexpr uint32_t kMaxInstanceLevels = 8;

Aabb prim_bbox(const Prim &p);
void build_bvh(Bvh &out, std::vector<Prim> &&prims);  // bvh.rs:300-327

// CRT_WIDE (A/B runs, tests): 1 asks for the four-wave kernels, 0 for the three-wave ones. A request the image cannot
// take falls back to the scene's own preference — the knob sweeps whole test sets, direct-leaf scenes included.
int wide_request();  // -1 unset

// Every A/B knob of the library. The environment is read in ONE place (scene.cpp, read_knobs) — when a scene image is
// flattened and when a renderer is created — validated and clamped there; nothing else in the library calls getenv.
// -1 = not set (the library's own choice). None of them changes a result (tests/test_gpu_render.py,
// test_round3_knobs_change_no_bit); profiles/README.md lists what each was measured for.
struct Knobs {
  // scene image (flatten_image)
  int pool_stack_deep = -1;   // CRT_POOL_STACK_RT: 1 the deep LDS split, 0 the flat one (any value >= 10 / below)
  int direct_leaves = -1;     // CRT_DIRECT_LEAVES
  int direct_inst = -1;       // CRT_DIRECT_INST (can only switch the form OFF)
  int stage_roots = -1;       // CRT_STAGE_ROOTS: at most n instanced roots in the LDS window
  uint32_t cold = 0;          // CRT_COLD: cold bits the image asks for on top of what it needs (0..7)
  int inst_order = 1;         // CRT_INST_ORDER
  int hot_packets = 1;        // CRT_HOT_PACKETS
  // engine choice
  int wide = -1;              // CRT_WIDE
  // renderer
  int mat_dedup = 1, partition = -1, simple = 1, prefer_stage = -1, cam_compact = 1, root_cull = -1, shade_wide = -1, shade_pipe = 1, fused = -1;
  int mat_derived = 1;        // CRT_MAT_DERIVED: 0 = the shade kernels compute the per-material constants at every vertex again
  int slim_state = 1;         // CRT_SLIM_STATE: 0 = the pipelined shade kernel hands itself the full path state
  int camera_trace = -1;      // CRT_CAMERA_TRACE: 0 never k_camera, 1 wherever allowed, 2 / 3 the test forms (PlanInputs), unset: the host rule
  int camera_vertex = -1;     // CRT_CAMERA_VERTEX: 0 never k_camera_vertex, 1 or unset wherever the plan's rule holds
  int pixel_table = -1;       // CRT_PIXEL_TABLE: 0 never the per-pixel camera table, 1 or unset wherever a camera launch runs
  int cull_root_lds = -1;     // CRT_CULL_ROOT_LDS: 0 the camera launch's cull holds the root in registers, 1 or unset reads it from LDS
  int noclassify_from = 1 << 30, tail_from = 12, lanes = 4, grid_mult = 0;
  size_t max_batch_slots = 0, lane_min_paths = (size_t)96 << 20, stage_min_paths = (size_t)96 << 20;
};
Knobs read_knobs();
inline int select_engine_env(const DevScene &s, EngineSelect &e, bool renderer = false) {
  if (select_engine(s, wide_request(), e, renderer) == CRT_OK) return CRT_OK;
  return select_engine(s, -1, e, renderer);
}

struct DeviceImage {
  void *blob = nullptr;
  size_t bytes[7] = {0, 0, 0, 0, 0, 0, 0};  // nodes, leaves, packets, indices, prims, instances, normals (+ placements of moving instances)
  uint32_t *err = nullptr;  // this scene's traversal error word (the blob's last 256 bytes): crt_scene_traversal_error
  DevScene view{};
  ~DeviceImage();
};

struct Scene : std::enable_shared_from_this<Scene> {
  Bvh bvh;
  uint32_t n_geoms = 0;
  bool has_motion = false;
  uint32_t depth = 1;  // levels of instancing below and including this scene: 1 = no instances
  std::mutex dev_mu;
  std::unique_ptr<DeviceImage> dev;  // built on first query
  int ensure_device();               // CRT_OK or CRT_ERR_NO_DEVICE
};

// Host-only self-check of the image Scene::ensure_device would upload (scene.cpp): CRT_OK and eight counts, or
// CRT_ERR_BAD_ARG with the broken invariant in crt_last_error.
int scene_image_check(const Scene &scene, uint64_t out[8]);
// Host-only: the image's primitive records (scene.cpp).
int scene_image_prims(const Scene &scene, std::vector<DevPrim> &out);
// Host-only: array `which` of the image (nodes, leaves, packets, indices, prims, instances, normals) as bytes, and the
// view's plain fields: root, has_packets, n_nodes, n_packets, direct_leaves, pool_stack, cold, 0 (scene.cpp).
int scene_image_array(const Scene &scene, uint32_t which, std::vector<unsigned char> &out, uint32_t view[8]);
// Host-only: node_touched on the root node of the image this scene would upload, for n rays of six floats (origin,
// direction): out[i] = 1 when ray i touches a child of the root. *root = the image's root (CRT_INVALID_ID: an empty
// scene, every out[i] = 0).
int scene_root_touched(const Scene &scene, const float *rays6, size_t n, float t_min, float t_max, uint8_t *out, uint32_t *root);
// Host-only: select_engine on the image this scene would upload, verified against a census of the image (scene.cpp).
int scene_engine_select(const Scene &scene, int want_wide, uint32_t out[8]);

enum GeomKind { G_MESH, G_SPHERE, G_INSTANCE, G_CURVES, G_CUBICS };
struct Geom {
  GeomKind kind = G_MESH;
  uint32_t mask = CRT_MASK_ALL;
  std::vector<float> verts;
  std::vector<uint32_t> idx;
  bool has_normals = false;
  std::vector<float> normals;
  F3 center{0, 0, 0};
  float radius = 0;
  std::vector<float> segs;  // G_CURVES: 8 floats per segment, p0 r0 p1 r1 (scene.rs:15-23)
                            // G_CUBICS: 14 floats per span, cp0 cp1 cp2 cp3 r0 r1 (scene.rs:70-80)
  std::shared_ptr<Scene> scene;
  Affine l2w{};
  bool has_end = false;
  Affine l2w_end{};
};

struct Builder { std::vector<Geom> geoms; };

std::shared_ptr<Scene> commit(Builder &&b);  // scene.rs:226-341

// ---------------------------------------------------------------------------------------------
// Device launches (kernels/traverse.hip)
// ---------------------------------------------------------------------------------------------
// d_err: device word the kernels OR their error bits into (1 = traversal stack overflow, 2 = instance nesting).
int launch_intersect_n(const DevScene &s, const CrtRay *d_rays, size_t n, float t_min, float t_max, CrtRayHit *d_hits,
                       void *stream, CrtTravStats *d_stats, uint32_t *d_err);
int launch_occluded_n(const DevScene &s, const CrtRay *d_rays, size_t n, float t_min, float t_max, uint32_t *d_out,
                      void *stream, CrtTravStats *d_stats, uint32_t *d_err);
int device_ok();
// Environment maps (environment.cpp). env_table_for_launch: the device table of live environments for a launch of the
// library's own, every live one uploaded first; *table = nullptr when none is live. env_retain: a reference to the
// environment with that id, or nothing when the id names none.
int env_table_for_launch(const void **table);
std::shared_ptr<void> env_retain(uint32_t id);
// Volume regions (volumes.cpp). volumes_build_image: VolumeRegion::new for every record and the image the seam kernels
// read, or CRT_ERR_BAD_ARG with the reason in crt_last_error. volumes_device: the device copy of a handle's image
// (uploaded on first use) as the pointers the kernels take.
namespace dev { struct VolRegionRec; }
struct VolumesView { const dev::VolRegionRec *regions = nullptr; const float *grid = nullptr; uint32_t n_regions = 0; };
int volumes_build_image(const CrtVolumeRegion *regions, size_t n, const float *grid, size_t grid_len, std::vector<unsigned char> &image);
int volumes_device(CrtVolumes *v, VolumesView &out);
// A handle is reference counted: crt_volumes_new hands the caller one reference, crt_volumes_free drops it, a renderer
// holds one of its own while the aggregate is bound (crt_renderer_set_volumes).
void volumes_retain(CrtVolumes *v);
void volumes_release(CrtVolumes *v);
uint32_t volumes_region_count(const CrtVolumes *v);
// printf-style text for crt_last_error() on this thread (failures that are not HIP calls).
void set_error_text(const char *fmt, ...);
// Nothing may unwind through the C ABI — a host in C or Rust cannot catch it, and unwinding into its frames is undefined:
// an entry point whose body allocates host memory (std containers) runs it through abi_guard; a failed allocation (or a
// length_error: crt_reserve(b, SIZE_MAX)) becomes CRT_ERR_NO_MEMORY with the reason in crt_last_error.
template <class F>
inline int abi_guard(const char *what, F &&body) noexcept {
  try { return body(); }
  catch (const std::exception &e) { set_error_text("%s: %s", what, e.what()); }
  catch (...) { set_error_text("%s: unknown failure", what); }
  return CRT_ERR_NO_MEMORY;
}

// Records the failing HIP call for crt_last_error() and returns false.
bool hip_failed(int /*hipError_t*/ err, const char *what, const char *file, int line);
#define CRT_HIP_OK(call) (!::crt::hip_failed((int)(call), #call, __FILE__, __LINE__))

}  // namespace crt

struct CrtScene { std::shared_ptr<crt::Scene> p; std::atomic<int> refs{1}; };
struct CrtBuilder { crt::Builder b; };
