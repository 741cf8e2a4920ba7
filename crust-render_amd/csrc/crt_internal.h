// Internal host/device declarations of libcrt_amd.so (not part of the ABI).
//
// Host side (C++17): geometry table, deterministic SBVH -> BVH4 build, flattening of a committed
// scene and everything it instances into ONE device image with absolute indices.
// Device side (HIP, gfx950): see kernels/.
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

// ---------------------------------------------------------------------------------------------
// Committed-tree records. These are the reference's layouts (bvh.rs:196-227, triangle.rs:182-196)
// and also the device layouts: one node = one 128-byte line, one packet = 192 bytes.
// ---------------------------------------------------------------------------------------------
struct alignas(16) WideNode {
  float bmin[3][4];
  float bmax[3][4];
  uint32_t child[4];
  uint32_t flags;  // bits 0-3 valid lane, bits 4-7 leaf lane
  uint32_t pad[3];
};
static_assert(sizeof(WideNode) == 128, "bvh.rs:1613-1616");

struct Leaf { uint32_t pkt_first, pkt_count, idx_first, idx_count; };
static_assert(sizeof(Leaf) == 16, "bvh.rs:220-227");

struct alignas(16) Tri4 {
  float v[3][3][4];  // [vertex][axis][lane]
  uint32_t prim[4];
  uint32_t active, mask_and, mask_or;
  uint32_t masks[4];
  // Device extra (the reference's padding word): bit k set iff lane k can produce a normal, i.e. it
  // has shading normals or a non-zero geometric cross product (prim.rs:76-86 rejects the others).
  uint32_t normal_ok;
};
static_assert(sizeof(Tri4) == 192, "triangle.rs:182-196");

// PRIM_CUBIC_TAIL: only in the device image — the second 64-byte record of a cubic span, never named by a leaf list.
enum PrimKind : uint32_t { PRIM_TRI = 0, PRIM_SPHERE = 1, PRIM_INSTANCE = 2, PRIM_CURVE = 3, PRIM_CUBIC = 4, PRIM_CUBIC_TAIL = 5 };

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
// flatness_depth (curve.rs:122-141) of a cubic span, cp = 12 floats, max_width = 2 * max(r0, r1) with the radii as
// given: l0, eps and x = SQRT_2 * 6 * l0 / (8 * eps) in f32 in the reference's order, then clamp(floor(log2(x) / 2), 0,
// 10) read exactly from x's binary exponent — no libm on the path. 0 when l0 <= 0, max_width <= 0, x is not finite or
// x < 1. The one function that computes it: commit stores it in the span's record, the kernels read it and loop.
uint32_t cubic_flatness_depth(const float cp[12], float max_width);
constexpr uint32_t kMaxCubicDepth = 10;  // curve.rs:98 MAX_RECURSION_DEPTH
void build_bvh(Bvh &out, std::vector<Prim> &&prims);  // bvh.rs:300-327

// ---------------------------------------------------------------------------------------------
// Device image (HBM): the queried scene and every scene it instances, flattened.
// ---------------------------------------------------------------------------------------------
struct DevPrim {  // 64 bytes
  uint32_t kind, geom_id, prim_id, mask;
  float d[12];  // tri: v0 v1 v2 (9), then flat: [9..11] = its unit geometric normal (flat_tri_normal)
                //                         smooth: [9] = shading-normal slot (u32 bits), [10] = kSmoothNormalTag
                // sphere: center (3), radius | instance: [0] = instance slot (u32 bits)
                // curve segment: p0 (3), r0, p1 (3), r1
                // cubic span: cp0 cp1 cp2 cp3 (12); the NEXT record (PRIM_CUBIC_TAIL, same header): r0, r1, depth (u32 bits)
};
static_assert(sizeof(DevPrim) == 64, "");
// DevPrim::d[10] of a triangle with shading normals: a SIGNALLING NaN. flat_tri_normal cannot produce it — an IEEE
// division returns a quiet NaN (bit 22 set) whatever its operands — so one word tells the two forms apart, and it is in
// the 16 bytes (d[8..11]) the normal is read from anyway.
constexpr uint32_t kSmoothNormalTag = 0x7fa5a5a5u;

#if defined(__HIPCC__)
#define CRT_HOST_DEVICE __host__ __device__
#else
#define CRT_HOST_DEVICE
#endif
// Unit geometric normal of a flat triangle (prim.rs:76-95): edges, cross product, sqrt of the dot product, three IEEE
// divisions, in the reference's operation order (-ffp-contract=off). A constant of the committed triangle: evaluated
// once per commit (scene.cpp, flatten_image) and stored in the primitive record; the kernels only read it. A zero-area
// triangle yields whatever the divisions give (NaN or infinities); it is never emitted (Tri4::normal_ok).
CRT_HOST_DEVICE inline void flat_tri_normal(const float v[9], float n[3]) {
  const float e1x = v[3] - v[0], e1y = v[4] - v[1], e1z = v[5] - v[2];
  const float e2x = v[6] - v[0], e2y = v[7] - v[1], e2z = v[8] - v[2];
  const float x = e1y * e2z - e2y * e1z;
  const float y = e1z * e2x - e2z * e1x;
  const float z = e1x * e2y - e2x * e1y;
  const float len = sqrtf((x * x + y * y) + z * z);
  n[0] = x / len; n[1] = y / len; n[2] = z / len;
}

// "Does this ray touch any child of this node": the node step of the traversal engine (kernels/traverse_pool.hip.h, the
// slab4 loop; RaySlab::slab4, bvh.rs:790-808) as one predicate on a device-form node (an empty lane's child word is
// CRT_INVALID_ID), with the engine's own expressions in the engine's order: the reciprocal direction of setup_ray
// (safe_inv3, bvh.rs:662-668), t0 = (lo - o) * inv, t1 = (hi - o) * inv, the min / max chains seeded with t_min / t_max,
// lane on iff tn <= tf. Identical expressions, so the two agree on every ray, NaN and infinite directions included
// (fminf / fmaxf return the operand that is a number on both sides). The renderer's generate stage asks it of the
// image's root for every camera ray (pathtrace.hip, generate_segment_cull): a ray that touches no child of the root is
// a ray the engine reports as a miss after exactly one node step. One source for host and device, as flat_tri_normal.
CRT_HOST_DEVICE inline float safe_inv(float d) {
  const float TINY = 1e-20f, HUGE_ = 1e20f;
  return fabsf(d) < TINY ? copysignf(HUGE_, d) : 1.0f / d;
}
CRT_HOST_DEVICE inline bool node_touched(const float bmin[3][4], const float bmax[3][4], const uint32_t child[4], float ox,
                                         float oy, float oz, float dx, float dy, float dz, float t_min, float t_max) {
  const float ix = safe_inv(dx), iy = safe_inv(dy), iz = safe_inv(dz);
  bool any = false;
  for (int l = 0; l < 4; l++) {
    const float t0x = (bmin[0][l] - ox) * ix, t1x = (bmax[0][l] - ox) * ix;
    const float t0y = (bmin[1][l] - oy) * iy, t1y = (bmax[1][l] - oy) * iy;
    const float t0z = (bmin[2][l] - oz) * iz, t1z = (bmax[2][l] - oz) * iz;
    const float tn = fmaxf(fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z)), t_min);
    const float tf = fminf(fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z)), t_max);
    any = any || ((tn <= tf) && child[l] != 0xFFFFFFFFu);
  }
  return any;
}

struct DevInstance {  // 64 bytes: what an instance entry reads (half a cache line; 40 000 placements stay L2-resident)
  float w2l[12];      // cached world-to-local at time 0 (prim.rs:266); its matrix3 transposed is the normal matrix (:267)
  uint32_t root;      // absolute node index of the instanced scene's root
  uint32_t flags;     // bit 0: the instanced tree has Tri4 packets; bit 1: transform motion blur (prim.rs:276);
                      // bits 2..31: float offset of its DevInstanceMotion in `normals` (moving instances only)
  uint32_t geom_id;   // the instance's own geometry id and ray mask: a leaf's index list addresses an instance
  uint32_t mask;      //   record directly (kIndexInstance), so entering one never touches its DevPrim
};
static_assert(sizeof(DevInstance) == 64, "");
// The two placements of a MOVING instance (prim.rs:285-331; flags bit 1), read only by a ray with a shutter time > 0:
// 24 floats in the `normals` array at float offset flags >> 2. (Not an array of its own: every pointer of DevScene
// is a pair of scalar registers live through the whole traversal, and the path kernels already spill those.)
struct DevInstanceMotion {
  float l2w[12];
  float l2w_end[12];
};
// Entries of `indices` (a leaf's scalar list): primitive index, or kIndexInstance | instance slot. Instance slots
// follow the order of the scalar lists, so the placements of one leaf, and of neighbouring leaves, share cache lines.
constexpr uint32_t kIndexInstance = 0x80000000u;
namespace dev { constexpr int kBlock = 256; }  // threads per workgroup (4 waves): the kernels' launch bounds and the hosts' launches

struct DevScene {
  const WideNode *nodes;
  const Leaf *leaves;
  const Tri4 *packets;
  const uint32_t *indices;
  const DevPrim *prims;
  const DevInstance *instances;
  const float *normals;  // 9 floats per smooth triangle; then 24 per moving instance
  uint32_t root;         // CRT_INVALID_ID when the scene is empty (bvh.rs:442-444)
  uint32_t has_packets;
  uint32_t n_nodes;      // numbered for the LDS window: top of the top-level tree, the instanced trees' roots, then
                         // the rest breadth-first (see Scene::ensure_device)
  uint32_t pool_stack;   // LDS stack entries per ray the traversal engine uses for this scene (6 flat, 10 instanced)
  uint32_t n_packets;    // Tri4 packets, the queried tree's first (scene.cpp rotates them there; crt_scene_image_check): the first ones are staged in LDS behind the node window
  uint32_t direct_leaves;  // leaves without packets and with 1-3 scalar entries are encoded in the child word (below)
  uint32_t cold;           // kCold* bits: the rarely used per-ray state a traversal of this scene can need (traverse_pool.hip.h)
};
// DevScene::cold. kColdUV: some triangle has shading normals (prim.rs:76-95 interpolates them with u, v). kColdNormal:
// a sphere exists somewhere (its normal is computed at the hit and kept until emit), or instances nest deeper than one
// level (a hit below the first level is taken to its parent's space at exit). kColdTime: a moving instance exists.
enum : uint32_t { kColdUV = 1u, kColdNormal = 2u, kColdTime = 4u, kColdAll = 7u };
// Outside kColdAll, a bit of DevScene::cold AND of the kernels' cold argument: some tree of the image holds a round
// curve segment (PRIM_CURVE). Only kernel instances built with it carry the rounded-cone arm of the scalar-primitive
// phase (traverse_pool.hip.h) — three-wave instances all; every other instance is compiled exactly as without curves.
// A curve's normal is computed at the hit and kept until emit, so the bit implies kColdNormal.
constexpr uint32_t kColdCurve = 16u;
// Outside kColdAll too: some tree of the image holds a cubic curve span (PRIM_CUBIC). It implies kColdCurve (and so
// kColdNormal): the instances built with it carry the span's subdivision walk BESIDE the rounded-cone arm — twelve
// more three-wave instances; a round-only curve image keeps the instances it had.
constexpr uint32_t kColdCubic = 32u;
// A fourth bit of the KERNELS' cold argument (never of DevScene::cold): the image holds no Tri4 packet at all and carries
// direct leaf words (a scene of analytic spheres: openpbr_showcase) — the kernel instance then holds ONE engine copy, the
// direct one, without the packet phase's Woop test and without the per-ray shear constants (traverse_pool.hip.h, NOPK).
constexpr uint32_t kNoPackets = 8u;
// Device child words of a node: inner child = node index; leaf child = kLeafTag | leaf index; empty lane =
// CRT_INVALID_ID. With DevScene::direct_leaves a leaf that holds no Tri4 packet and one to three scalar entries
// (spheres, instances: every leaf of an instanced city's top-level tree) is written as
//   kLeafTag | kDirectLeafTag | count << 28 | idx_first                    entries indices[idx_first ..)
//   kLeafTag | kDirectLeafTag | count << 28 | kDirectInstTag | slot       entries = instances slot, slot + 1, ..
// so the ray goes from the node straight to the scalar list: no 16-byte Leaf fetch, no packet step that finds
// nothing and, when the entries are instances in consecutive slots, no index fetch either. Chosen per scene at
// upload (instance-heavy or packet-free scenes), like the LDS split.
constexpr uint32_t kDirectLeafTag = 0x40000000u;
constexpr uint32_t kDirectInstTag = 0x08000000u;
constexpr uint32_t kDirectIndexMask = 0x07ffffffu;
// Nodes of the top of the tree the traversal kernels stage in LDS per workgroup (kernels/traverse_pool.hip.h): the
// upload numbers the nodes for this window.
#ifndef CRT_POOL_NODES_WIDE
#define CRT_POOL_NODES_WIDE 26  // the four-workgroups-per-CU kernels (small flat scenes)
#endif
#ifndef CRT_POOL_NODES_WIDE_DEEP
#define CRT_POOL_NODES_WIDE_DEEP 12  // ... of the four-wave kernels on a large tree or an instance-heavy scene (they trade the window for stack
                                     // entries; 12 is what the 40 KB arena has left beside five entries: MedCity's root + its 8 prototype roots fit, +1.3 % over 8)
#endif
#ifndef CRT_DIRECT_INST
#define CRT_DIRECT_INST 1  // 0: the direct-instance form is neither written nor understood (A/B builds)
#endif
#ifndef CRT_POOL_NODES
#define CRT_POOL_NODES 72
#endif
#ifndef CRT_POOL_NODES_DEEP
#define CRT_POOL_NODES_DEEP 16  // with the deep stack: 16 still fit three workgroups per CU (+0.4 %); 24 do not (-33 %)
#endif
#ifndef CRT_WIDE_DIRECT_BUILD
#define CRT_WIDE_DIRECT_BUILD 1  // four-wave kernel instances with the direct engine copy (WIDE = 2); CRT_WIDE=2 asks for them
#endif
#ifndef CRT_NOPK_BUILD
// 1: packet-free instances of the fused kernel for images without a Tri4 packet (kNoPackets). Measured on openpbr_showcase
// (round 4): one engine copy and 13 % fewer instructions, but 53 -> 67 spilled registers in k_path<2, true, .>: 12 294 ->
// 12 176 Mray/s. Off; the switch stays for A/B builds.
#define CRT_NOPK_BUILD 0
#endif
#ifndef CRT_DIRECT_LEAVES
#define CRT_DIRECT_LEAVES 1  // 0: neither written by the upload nor understood by the engine (A/B builds)
#endif

// Which scenes the four-workgroups-per-CU traversal kernels (kernels/traverse_pool.hip.h, WIDE: three stack entries
// per ray in LDS) are launched for: flat (not instance-heavy) triangle scenes whose trees are shallow enough for that
// stack. Measured (profiles/README.md): the renderer's per-stage pipeline on them gains 4-9 % on cornellbox, veach_mis,
// sun_sky (at most a few hundred nodes); 16 M incoherent rays against 43 200 triangles (3 600 nodes, 15 nodes per ray)
// lose 7 %, an instanced city 6 %, sphere-only scenes are indifferent.
// ... and only images WITHOUT direct child words: the four-wave kernels are built without the direct-leaf engine copy
// (run_traversal), so a direct word would be read as a leaf index (the round-3 fault, profiles/README.md).
// Round 4: LARGE flat trees too, in the renderer — its four-wave kernels keep no mask plane and split their arena by tree
// (five stack entries + a twelve-node window; traverse_pool.hip.h): the reference's stress scene 2538 -> 2738 Mray/s
// (+7.9 %), the 7 M-triangle synthetic scene +0.7 %. The batched queries (one stack entry less: per-ray masks) keep the
// three-wave kernels on those trees, as do the mid-size ones (1 024 < nodes <= 2 048: the flat 6 + 72 split).
inline bool wide_split(const DevScene &s, bool renderer = false) {
  if (s.direct_leaves != 0 || s.n_packets == 0) return false;
  if (s.pool_stack >= 10u) return renderer && s.n_nodes > 2048u;  // the deep split chosen for a large tree, not for instances
  return s.n_nodes <= 1024u;
}

// LDS stack entries per ray of the three engine splits (kernels/traverse_pool.hip.h sizes its arenas from these).
#ifndef CRT_POOL_STACK
#define CRT_POOL_STACK 6        // flat scenes, three-wave kernels
#endif
#ifndef CRT_POOL_STACK_DEEP
#define CRT_POOL_STACK_DEEP 10  // instance-heavy scenes and large trees, three-wave kernels
#endif
#ifndef CRT_POOL_STACK_WIDE
#define CRT_POOL_STACK_WIDE 3   // four-wave kernels
#endif

// Which instance of the traversal engine runs an image. THE one decision: the renderer (render.cpp), the batched and
// the single-ray queries (traverse.hip) and the host-only crt_scene_engine_select all call select_engine, and every
// launch goes through the EngineSelect it returns — an engine instance never meets an image form it was not built for
// (rounds 2 and 3 each lost a GPU box to exactly that: profiles/README.md, "The r02f abort", "The r03w fault").
struct EngineSelect {
  bool wide = false;       // the four-workgroups-per-CU kernels (WIDE): the flat engine copy, 3-5 LDS stack entries (lds_stack)
  bool wide_direct = false;  // ... their instances that hold the DIRECT engine copy only (WIDE = 2): direct-leaf images
  bool direct = false;     // the DIRECT engine copy of the three-wave kernels: reads direct child words, root test at entry
  uint32_t lds_stack = CRT_POOL_STACK;  // stack entries per ray in LDS
  uint32_t window = CRT_POOL_NODES;     // nodes staged in LDS per workgroup
  int ext_cold = (int)kColdAll;         // k_extend<., ., COLD>: none / the pending normal only / everything
  int path_cold = (int)kColdAll;        // k_path<., ., COLD> of simple scenes: none / everything
  bool curve = false;      // the image holds curve segments: the three-wave instances with the rounded-cone arm (kColdCurve)
  bool cubic = false;      // ... and cubic spans: their instances with the subdivision walk as well (kColdCubic; implies curve)
  int curve_cold() const { return (int)((curve ? kColdCurve : 0u) | (cubic ? kColdCubic : 0u)); }
};
// want_wide: -1 = the scene's own preference (wide_split), 0 / 1 = asked for (CRT_WIDE, tests); renderer: the choice for
// the renderer's kernels (the batched queries' differs on large trees, wide_split). CRT_OK, or
// CRT_ERR_UNSUPPORTED when what was asked for cannot decode the image — nothing is launched then.
inline int select_engine(const DevScene &s, int want_wide, EngineSelect &e, bool renderer = false) {
  const bool has_direct_words = s.direct_leaves != 0;
  const bool curve = (s.cold & kColdCurve) != 0;
  if (curve && want_wide > 0) return CRT_ERR_UNSUPPORTED;  // no four-wave instance carries the rounded-cone arm
  // the plain WIDE kernels carry no direct-leaf engine; their WIDE = 2 instances (the renderer's only) carry nothing else
  if (want_wide == 1 && has_direct_words) return CRT_ERR_UNSUPPORTED;
  if (want_wide == 2 && !(has_direct_words && renderer && CRT_DIRECT_LEAVES != 0 && CRT_WIDE_DIRECT_BUILD != 0)) return CRT_ERR_UNSUPPORTED;
  // Round 4: the renderer runs DIRECT-LEAF images (instance-heavy or packet-free scenes) on the four-wave kernels too, on
  // instances that hold the direct engine copy only — an entry the root test rejects never touches the stack, so the
  // direct engine lives with the short LDS stack where the flat one (gauged at 1 985 against 1 977 on MedCity) did not:
  // PointInstancedMedCity 2 234 -> 2 285 Mray/s, openpbr_showcase 13 070 -> 14 045, a 32 761-instance city 2 599 -> 2 790.
  const bool auto_wide_direct = !curve && want_wide < 0 && renderer && has_direct_words && CRT_DIRECT_LEAVES != 0 && CRT_WIDE_DIRECT_BUILD != 0;
  e.wide = auto_wide_direct || (want_wide < 0 ? (!curve && wide_split(s, renderer)) : want_wide != 0);
  e.wide_direct = auto_wide_direct || want_wide == 2;
  e.direct = (!e.wide || e.wide_direct) && CRT_DIRECT_LEAVES != 0 && has_direct_words;
  if (has_direct_words && !e.direct) return CRT_ERR_UNSUPPORTED;      // (a build without the direct form never writes one)
  const bool deep = s.pool_stack >= (uint32_t)CRT_POOL_STACK_DEEP;    // run_traversal's rule
  // (the wide arena's splits: the renderer's kernels, which keep no mask plane; the batched queries have one entry less)
  e.lds_stack = e.wide ? (uint32_t)CRT_POOL_STACK_WIDE + 1u + (deep ? 1u : 0u) : (deep ? (uint32_t)CRT_POOL_STACK_DEEP : (uint32_t)CRT_POOL_STACK);
  e.window = e.wide ? (deep ? (uint32_t)CRT_POOL_NODES_WIDE_DEEP : (uint32_t)CRT_POOL_NODES_WIDE)
                    : (deep ? (uint32_t)CRT_POOL_NODES_DEEP : (uint32_t)CRT_POOL_NODES);
  const int cold = (int)(s.cold & kColdAll);
  e.ext_cold = cold == 0 ? 0 : (cold == (int)kColdNormal ? (int)kColdNormal : (int)kColdAll);
  e.path_cold = cold == 0 ? 0 : (int)kColdAll;
  // a packet-free image with direct words: the fused kernel's packet-free instance (general materials; pathtrace.hip)
  if (CRT_NOPK_BUILD && s.n_packets == 0 && e.direct) e.path_cold = (int)(kColdAll | kNoPackets);
  e.curve = curve;
  e.cubic = curve && (s.cold & kColdCubic) != 0;
  if (curve) e.ext_cold = e.path_cold = (int)kColdAll | e.curve_cold();  // one instance each: everything + the arm(s)
  return CRT_OK;
}
// The check every launch site makes on the EngineSelect it was handed (defence in depth: select_engine already
// guarantees it): the instance can decode every child word of the image and keeps every cold field the image can need.
inline bool engine_accepts(const EngineSelect &e, const DevScene &s, int kernel_cold) {
  if (s.direct_leaves != 0 && ((e.wide && !e.wide_direct) || !e.direct)) return false;
  if (e.wide_direct && s.direct_leaves == 0) return false;
  if ((kernel_cold & (int)kNoPackets) && (s.n_packets != 0 || s.direct_leaves == 0)) return false;  // a packet-free instance on packets
  if ((s.cold & kColdCurve) && (e.wide || !e.curve)) return false;  // a curve image on an instance without the arm
  if ((s.cold & kColdCubic) && (e.wide || !e.cubic || !(s.cold & kColdCurve))) return false;  // ... without the span's walk
  return ((int)(s.cold & (kColdAll | kColdCurve | kColdCubic)) & ~kernel_cold) == 0;
}

// ---------------------------------------------------------------------------------------------
// The renderer's launch plan: which kernel instances run one batch. plan_launches decides it once per batch from a
// PlanInputs — every fact the choice depends on, as plain values — and names each instance by an InstanceKey;
// kernels/pathtrace.hip holds the table {key, kernel pointer} built from the lists below (resolve_kernels,
// render_kernels.h), and render.cpp launches through what that finds there. A new instance is one row of a list and one
// line of policy in plan_launches. Plain C++17, no HIP names:
// tests/test_launch_plan.py sweeps the function on the CPU.
// ---------------------------------------------------------------------------------------------
enum KernelFamily : uint8_t { KF_NONE = 0, KF_EXTEND, KF_PATH, KF_SHADE, KF_SHADE_ENV, KF_SHADE_PIPE, KF_SHADOW, KF_SHADOW_CURVE, KF_SHADOW_CUBIC,
                               KF_SHADE_VOL, KF_VOLUME, KF_SHADOW_VOLUME, KF_EXTEND_DEFERRED, KF_CAMERA, KF_CAMERA_VERTEX,
                               KF_EXTEND_FACES, KF_SHADE_FACES };
struct InstanceKey {  // a kernel template and its arguments, in the template's order (bools as 0 / 1)
  uint8_t family = KF_NONE;
  uint8_t arg[5] = {0, 0, 0, 0, 0};
  bool none() const { return family == KF_NONE; }
  bool operator==(const InstanceKey &o) const {
    return family == o.family && arg[0] == o.arg[0] && arg[1] == o.arg[1] && arg[2] == o.arg[2] && arg[3] == o.arg[3] && arg[4] == o.arg[4];
  }
};
#define CRT_INSTANCE_KEY(family, kernel, ...) ::crt::InstanceKey{::crt::KF_##family, {__VA_ARGS__}}
// Every instance of a multi-form kernel this build holds, one list per kernel signature: X(family, kernel, template
// arguments...). The cold arguments are written as numbers: 2 = kColdNormal, 7 = kColdAll, 15 = kColdAll | kNoPackets,
// 23 = kColdAll | kColdCurve, 55 = kColdAll | kColdCurve | kColdCubic.
#if CRT_WIDE_DIRECT_BUILD  // the four-wave instances with the direct engine copy (WIDE = 2)
#define CRT_WIDE_DIRECT_INSTANCES_EXTEND(X) X(EXTEND, k_extend, false, 2, 0) X(EXTEND, k_extend, false, 2, 2) X(EXTEND, k_extend, false, 2, 7)
#define CRT_WIDE_DIRECT_INSTANCES_SHADOW(X) X(SHADOW, k_shadow, false, 2)
#else
#define CRT_WIDE_DIRECT_INSTANCES_EXTEND(X)
#define CRT_WIDE_DIRECT_INSTANCES_SHADOW(X)
#endif
#if CRT_NOPK_BUILD  // the packet-free instances of the fused kernel exist only in builds that ask for them
#define CRT_NOPK_INSTANCES_PATH(X) X(PATH, k_path, 1, false, 15, false) X(PATH, k_path, 1, true, 15, false) X(PATH, k_path, 2, false, 15, false) X(PATH, k_path, 2, true, 15, false)
#else
#define CRT_NOPK_INSTANCES_PATH(X)
#endif
#define CRT_INSTANCES_EXTEND(X) /* k_extend<STATS, WIDE, COLD> */ \
  X(EXTEND, k_extend, false, 0, 0) X(EXTEND, k_extend, false, 0, 2) X(EXTEND, k_extend, false, 0, 7) \
  X(EXTEND, k_extend, false, 1, 0) X(EXTEND, k_extend, false, 1, 2) X(EXTEND, k_extend, false, 1, 7) \
  CRT_WIDE_DIRECT_INSTANCES_EXTEND(X) \
  X(EXTEND, k_extend, true, 0, 7) X(EXTEND, k_extend, true, 1, 7) \
  X(EXTEND, k_extend, false, 0, 23) X(EXTEND, k_extend, true, 0, 23) X(EXTEND, k_extend, false, 0, 55) X(EXTEND, k_extend, true, 0, 55)
// k_extend_deferred<STATS, WIDE, COLD>: the first-bounce traversal behind k_camera (LaunchPlan::camera_trace) — the pool
// engine over the per-segment list of the camera rays k_camera deferred. A list of its own: a plan names the instance
// through extend_deferred_key(), never in `extend`.
#define CRT_INSTANCES_EXTEND_DEFERRED(X) /* k_extend_deferred<STATS, WIDE, COLD> */ \
  X(EXTEND_DEFERRED, k_extend_deferred, false, 1, 0)
#define CRT_INSTANCES_PATH(X) /* k_path<MATS, LIT, COLD, DRV>: simple-material tables (derived records or raw), then general ones */ \
  X(PATH, k_path, 0, false, 0, true) X(PATH, k_path, 0, false, 7, true) X(PATH, k_path, 0, true, 0, true) X(PATH, k_path, 0, true, 7, true) \
  X(PATH, k_path, 0, false, 0, false) X(PATH, k_path, 0, false, 7, false) X(PATH, k_path, 0, true, 0, false) X(PATH, k_path, 0, true, 7, false) \
  X(PATH, k_path, 1, false, 7, false) X(PATH, k_path, 1, false, 23, false) X(PATH, k_path, 1, false, 55, false) \
  X(PATH, k_path, 1, true, 7, false) X(PATH, k_path, 1, true, 23, false) X(PATH, k_path, 1, true, 55, false) \
  X(PATH, k_path, 2, false, 7, false) X(PATH, k_path, 2, false, 23, false) X(PATH, k_path, 2, false, 55, false) \
  X(PATH, k_path, 2, true, 7, false) X(PATH, k_path, 2, true, 23, false) X(PATH, k_path, 2, true, 55, false) \
  CRT_NOPK_INSTANCES_PATH(X)
#define CRT_INSTANCES_SHADE(X) /* k_shade<MATS, INF, WIDE, LIT, DRV>, k_shade_env<MATS, DRV> */ \
  X(SHADE, k_shade, 0, false, false, false, true) X(SHADE, k_shade, 0, false, false, true, true) X(SHADE, k_shade, 0, false, true, false, true) \
  X(SHADE, k_shade, 0, false, true, true, true) X(SHADE, k_shade, 0, true, false, true, true) \
  X(SHADE, k_shade, 0, false, false, false, false) X(SHADE, k_shade, 0, false, false, true, false) X(SHADE, k_shade, 0, false, true, false, false) \
  X(SHADE, k_shade, 0, false, true, true, false) X(SHADE, k_shade, 0, true, false, true, false) \
  X(SHADE, k_shade, 1, false, false, false, false) X(SHADE, k_shade, 1, false, false, true, false) X(SHADE, k_shade, 1, true, false, true, false) \
  X(SHADE, k_shade, 2, false, false, false, false) X(SHADE, k_shade, 2, false, false, true, false) X(SHADE, k_shade, 2, true, false, true, false) \
  X(SHADE_ENV, k_shade_env, 0, true) X(SHADE_ENV, k_shade_env, 0, false) X(SHADE_ENV, k_shade_env, 1, false) X(SHADE_ENV, k_shade_env, 2, false)
#define CRT_INSTANCES_SHADE_PIPE(X) /* k_shade_pipe<DRV> */ \
  X(SHADE_PIPE, k_shade_pipe, true) X(SHADE_PIPE, k_shade_pipe, false)
// k_shade_pipe<DRV, true>: the instances that carry the slim path state between two of their launches (LaunchPlan::
// slim_state). A list of their own: a plan names them through shade_slim_key(), never in shade_early.
#define CRT_INSTANCES_SHADE_PIPE_SLIM(X) /* k_shade_pipe<DRV, SLIM> */ \
  X(SHADE_PIPE, k_shade_pipe, true, true) X(SHADE_PIPE, k_shade_pipe, false, true)
#define CRT_INSTANCES_SHADOW(X) /* k_shadow<STATS, WIDE>, k_shadow_curve<STATS>, k_shadow_cubic<STATS> */ \
  X(SHADOW, k_shadow, false, 0) X(SHADOW, k_shadow, false, 1) CRT_WIDE_DIRECT_INSTANCES_SHADOW(X) X(SHADOW, k_shadow, true, 0) X(SHADOW, k_shadow, true, 1) \
  X(SHADOW_CURVE, k_shadow_curve, false) X(SHADOW_CURVE, k_shadow_curve, true) X(SHADOW_CUBIC, k_shadow_cubic, false) X(SHADOW_CUBIC, k_shadow_cubic, true)
// k_shade_vol<MATS, INF, LIT>: the shade instances of volume renders (PlanInputs::volumes) — three waves, raw material
// records; INF 0 none / 1 distant lights and uniform domes / 2 mapped domes too. k_volume and k_shadow_volume have one
// form each: their keys carry the family alone.
#define CRT_INSTANCES_SHADE_VOL(X) /* k_shade_vol<MATS, INF, LIT> */ \
  X(SHADE_VOL, k_shade_vol, 0, 0, false) X(SHADE_VOL, k_shade_vol, 0, 0, true) X(SHADE_VOL, k_shade_vol, 0, 1, true) X(SHADE_VOL, k_shade_vol, 0, 2, true) \
  X(SHADE_VOL, k_shade_vol, 1, 0, false) X(SHADE_VOL, k_shade_vol, 1, 0, true) X(SHADE_VOL, k_shade_vol, 1, 1, true) X(SHADE_VOL, k_shade_vol, 1, 2, true) \
  X(SHADE_VOL, k_shade_vol, 2, 0, false) X(SHADE_VOL, k_shade_vol, 2, 0, true) X(SHADE_VOL, k_shade_vol, 2, 1, true) X(SHADE_VOL, k_shade_vol, 2, 2, true)
// Textured renders (PlanInputs::faces, crt_renderer_set_face_textures). k_extend_faces<WIDE, COLD>: k_extend whose emit also
// writes the hit's (prim_id, u, v) record — the engine width select_engine picked, the cold state that carries u, v
// (kColdAll, with the curve arms where the image holds curves). k_shade_faces<MATS, INF, LIT>: the shade instances over
// the MatFace view, instantiated like k_shade_vol's — three waves, raw material records. Lists of their own: a plan
// names them in `extend` / `shade` with these families.
#if CRT_WIDE_DIRECT_BUILD
#define CRT_WIDE_DIRECT_INSTANCES_EXTEND_FACES(X) X(EXTEND_FACES, k_extend_faces, 2, 7)
#else
#define CRT_WIDE_DIRECT_INSTANCES_EXTEND_FACES(X)
#endif
#define CRT_INSTANCES_EXTEND_FACES(X) /* k_extend_faces<WIDE, COLD> */ \
  X(EXTEND_FACES, k_extend_faces, 0, 7) X(EXTEND_FACES, k_extend_faces, 1, 7) CRT_WIDE_DIRECT_INSTANCES_EXTEND_FACES(X) \
  X(EXTEND_FACES, k_extend_faces, 0, 23) X(EXTEND_FACES, k_extend_faces, 0, 55)
#define CRT_INSTANCES_SHADE_FACES(X) /* k_shade_faces<MATS, INF, LIT> */ \
  X(SHADE_FACES, k_shade_faces, 0, 0, false) X(SHADE_FACES, k_shade_faces, 0, 0, true) X(SHADE_FACES, k_shade_faces, 0, 1, true) X(SHADE_FACES, k_shade_faces, 0, 2, true) \
  X(SHADE_FACES, k_shade_faces, 1, 0, false) X(SHADE_FACES, k_shade_faces, 1, 0, true) X(SHADE_FACES, k_shade_faces, 1, 1, true) X(SHADE_FACES, k_shade_faces, 1, 2, true) \
  X(SHADE_FACES, k_shade_faces, 2, 0, false) X(SHADE_FACES, k_shade_faces, 2, 0, true) X(SHADE_FACES, k_shade_faces, 2, 1, true) X(SHADE_FACES, k_shade_faces, 2, 2, true)
// The camera launches (LaunchPlan::camera_trace / camera_vertex): TABLE = the sample loop reads the per-pixel table,
// ROOT_LDS = the cull reads the root from the LDS window, DRV = shade_early's table. Lists of their own: a plan names
// the instance through camera_key().
#define CRT_INSTANCES_CAMERA(X) /* k_camera<TABLE, ROOT_LDS> */ \
  X(CAMERA, k_camera, false, false) X(CAMERA, k_camera, false, true) X(CAMERA, k_camera, true, false) X(CAMERA, k_camera, true, true)
#define CRT_INSTANCES_CAMERA_VERTEX(X) /* k_camera_vertex<DRV, TABLE, ROOT_LDS> */ \
  X(CAMERA_VERTEX, k_camera_vertex, false, false, false) X(CAMERA_VERTEX, k_camera_vertex, false, false, true) \
  X(CAMERA_VERTEX, k_camera_vertex, false, true, false) X(CAMERA_VERTEX, k_camera_vertex, false, true, true) \
  X(CAMERA_VERTEX, k_camera_vertex, true, false, false) X(CAMERA_VERTEX, k_camera_vertex, true, false, true) \
  X(CAMERA_VERTEX, k_camera_vertex, true, true, false) X(CAMERA_VERTEX, k_camera_vertex, true, true, true)

// What the choice of a batch's kernels depends on. The renderer keeps one: the engine choice, the A/B knobs and the
// build's switches are filled when it is created; what its Params hold, and the per-batch fields, before every plan.
struct PlanInputs {
  EngineSelect engine;     // which traversal-engine instance runs the image (select_engine)
  DevScene scene{};        // read: root, direct_leaves, n_packets, cold
  int mats_kind = 1;       // 0 simple / 1 general / 2 general with interior media: which instance of the shading code runs
  bool mat_derived = true; // CRT_MAT_DERIVED: simple-material tables launch the instances that read the derived records
  uint32_t n_lights = 0;
  bool has_inf_lights = false, has_env = false;  // a light at infinity; a mapped dome among them
  uint32_t strategy = 0;   // CRT_STRATEGY_*
  bool has_motion = false, lens = false;         // a moving instance; lens radius > 0
  bool mat_index = false;  // the material table is deduplicated (Params::mat_index)
  uint32_t partition = 0, class_stats = 0, n_materials = 0, max_depth = 0;
  // Two pipelines: FUSED — the whole path loop of a batch in one launch (k_path, three workgroups per CU) — and PER-STAGE
  // with the traversal kernels select_engine names. Every scene prefers one launch per stage for large batches: the
  // lanes then overlap launches of different stages and bounces, which one fused launch per lane cannot; the 2-3
  // launches per bounce cost ~0.8 ms per batch, worth it from `stage_min_paths` paths up (cornellbox 1080p, fused /
  // per-stage Mray/s: 66 M paths 7507 / 7300, 133 M 7658 / 7900). CRT_FUSED / CRT_PREFER_STAGE / CRT_STAGE_MIN_PATHS override.
  int force_fused = -1;
  bool prefer_stage = true;
  size_t stage_min_paths = (size_t)96 << 20;
  int tail_from = 12;             // CRT_TAIL_FROM: the bounce from which a per-stage batch finishes in one fused launch (0: never)
  int noclassify_from = 1 << 30;  // CRT_NOCLASSIFY_FROM: per-stage shade without its CLASSIFY pass from this bounce on
  int shade_wide = -1;            // CRT_SHADE_WIDE: 0 = the three-wave shade kernels even beside four-wave traversal kernels (A/B)
  int shade_pipe = 1;             // CRT_SHADE_PIPE: 0 = never the pipelined four-wave shade kernel (A/B, tests)
  int slim_state = 1;             // CRT_SLIM_STATE: 0 = the pipelined kernel carries the full path state between its launches (A/B, tests)
  bool no_emitter = false;        // no record of the material table can emit (table_has_no_emitter, at creation)
  bool cam_compact_ok = true;     // CRT_CAM_COMPACT
  int root_cull_knob = -1;        // CRT_ROOT_CULL: 0 = generate never finishes a camera ray, 1 = wherever the rule allows (A/B, tests)
  float root_miss_share = 0.0f;   // share of a coarse grid of camera rays that misses every child of the root (render.cpp)
  // A volume aggregate is bound (crt_renderer_set_volumes): the batch runs one launch per stage whatever its size, with
  // k_volume between extend and shade, the VOL shade instances and — where the shadow stage runs — k_shadow_volume ahead
  // of k_shadow. false: exactly the plan of a renderer that never heard of volumes.
  bool volumes = false;
  // A per-face texture aggregate is bound (crt_renderer_set_face_textures): one launch per stage whatever the batch size,
  // the FACES extend instance (its emit keeps prim_id, u, v per hit) and the FACES shade instances (MatFace). No fused
  // kernel and no tail, no camera-trace / camera-vertex / pixel-table launch, no pipelined or slim shade, no derived
  // material table; material_texture is indexed by geom_id whether or not the material table is deduplicated.
  // Not with volumes and not in the stats build: refused. false: exactly the plan of a renderer that never heard of it.
  bool faces = false;
  // CRT_CAMERA_TRACE: 0 = generate and the first extend as before, 1 = k_camera wherever the result allows, 2 / 3 = the
  // same with every surviving ray deferred / with a one-entry stack (tests: the list and the deferred instance), -1 = the
  // host rule below
  int camera_trace_knob = -1;
  // per batch
  size_t total = 0;               // paths of the batch
  bool stats = false;             // the stats build (crt_render_samples_stats)
  bool partial_active = false;    // adaptive stopping with an active list shorter than the frame (Params::active)
  // the build's switches that gate forms (kernels/pathtrace.hip, handed over in render_kernels.h's KernelBuild)
  bool cam_compact_build = true, wide_direct_build = CRT_WIDE_DIRECT_BUILD != 0, nopk_build = CRT_NOPK_BUILD != 0;
  bool shade_pipe_build = true, root_cull_build = true;
  int pipe_mat_max = 0;
  bool camera_trace_build = true;
  // CRT_CAMERA_VERTEX: 0 = k_camera and a first shade over every camera path, 1 / -1 (unset) = k_camera_vertex wherever
  // the rule below holds
  int camera_vertex_knob = -1;
  // CRT_PIXEL_TABLE: 0 = the camera launches compute a sample's per-pixel words every time, 1 / -1 (unset) = they read
  // the renderer's per-pixel table wherever one was built (pixel_table_ready: creation found a plan that could use it
  // and the memory for it)
  int pixel_table_knob = -1;
  bool pixel_table_ready = false;
  // CRT_CULL_ROOT_LDS: 1 / -1 (unset) = the camera launch's cull reads the root node from its LDS window every round,
  // 0 = it holds the root's 28 words in scalar registers, which the kernel parks in VGPR lanes (profiles/README.md)
  int cull_root_lds_knob = -1;
};
// k_camera traces every camera ray in the lane that made it against a window of the tree's top in LDS and a stack of
// kCamStack entries; a ray that needs more is traced a second time by the pool engine. That pays on the small flat trees
// whose camera rays rarely leave the window (cornellbox: profiles/README.md). Larger trees run the parent's launches
// unless CRT_CAMERA_TRACE=1 asks.
constexpr uint32_t kCameraTraceMaxNodes = 1024;
// The root cull pays where at least an eighth of the frame shows background: between the share that lost and the shares
// that won (profiles/README.md — cornellbox, 0.44 of its camera rays culled, +1.7 %; openpbr_showcase, 0.23, +1 %;
// veach_mis, 0.06, and the two scenes that fill their frame lose 1-3 %).
constexpr float kRootCullMinShare = 0.125f;
// The pipelined shade kernel serves unlit simple-material scenes of one material class whose whole material table fits
// the arena beside the staging blocks (pipe_mat_max); every other scene keeps k_shade with its LDS-resident table.
inline bool shade_pipe_fits(const PlanInputs &q) {
  return q.shade_pipe_build && q.shade_pipe != 0 && q.mats_kind == 0 && q.n_lights == 0 && !q.has_motion && !q.mat_index &&
         q.partition == 0 && !q.class_stats && q.n_materials <= (uint32_t)q.pipe_mat_max;
}
// True where NO record of a material table can emit: radiance gathered along a path is then +0 at every vertex, and the
// pipelined shade kernel need not carry it. A sufficient condition without arithmetic — a record's emission is
// emission_color for an Emissive and emission_color * emission_luminance for every other kind (shade.hip.h, emission()):
// either all three colour components compare equal to 0 (and the luminance they are multiplied by is finite), or a
// non-Emissive record has luminance 0 and a finite colour. A NaN anywhere fails both, so it counts as an emitter.
inline bool table_has_no_emitter(const CrtMaterial *m, size_t n) {
  auto finite = [](float x) { return x - x == 0.0f; };  // false for NaN and the infinities
  for (size_t k = 0; k < n; k++) {
    const float *c = m[k].emission_color, lum = m[k].emission_luminance;
    const bool emissive = m[k].kind == CRT_MAT_EMISSIVE;
    const bool black = c[0] == 0.0f && c[1] == 0.0f && c[2] == 0.0f && (emissive ? lum == lum : finite(lum));
    const bool dark = !emissive && lum == 0.0f && finite(c[0]) && finite(c[1]) && finite(c[2]);
    if (!black && !dark) return false;
  }
  return true;
}
// Material class = which arms of the vertex code a hit on this material runs (openpbr.rs:1026-1136 dispatches one of
// five lobes + thin film + dispersion per lane; rt_world.rs:219-231 binds the material per geom_id). Waves whose
// 64 vertices share a class skip the other classes' lobes with a scalar branch instead of idling through them.
//   0 emissive (Emissive: emission only, never scatters)      1 base: diffuse + specular (dielectric or metal)
//   2 layered: coat and / or fuzz and / or thin film on top    3 transmissive or subsurface (refraction, interior medium)
inline uint8_t material_class(const CrtMaterial &m) {
  if (m.kind == CRT_MAT_EMISSIVE) return 0;
  if (m.transmission_weight > 0.0f || m.subsurface_weight > 0.0f) return 3;
  if (m.coat_weight > 0.0f || m.fuzz_weight > 0.0f || m.thin_film_weight > 0.0f) return 2;
  return 1;
}
struct LaunchPlan {
  bool fused = true;              // one k_path launch for the whole path loop; otherwise one launch per stage and bounce
  bool wide = false;              // per-stage: the four-wave traversal kernels
  uint32_t tail_at = 0xffffffffu; // per-stage: the bounce from which k_path finishes the batch (0xffffffff: never)
  uint32_t cam_compact = 0;       // Params::cam_compact: 0 / 1 = camera paths as 16-byte records / 2 = with plane d beside them
  bool root_cull = false;         // generate finishes the camera rays that miss the root's boxes
  bool shadow = false;            // the shadow stage runs: a light list and a strategy that samples it
  int noclassify_from = 1 << 30;  // the bounce from which shade drops CLASSIFY
  int ext_cold = 0, path_cold = 0;  // the cold arguments the closest-hit kernels were chosen for (the refusal's text)
  InstanceKey path, extend, shade, shade_early, shadow_key;  // path: the fused launch or the tail; shade_early: the
                                  // pipelined instance, which runs the bounces before noclassify_from; none = not launched
  bool shade_piped() const { return !shade_early.none(); }
  // The pipelined kernel's launches hand each other the SLIM path state (render_kernels.h, PathSoA): three planes,
  // without the words every live path of a launch shares and without the radiance, which is +0 where nothing emits. A
  // field of its own — shade_early names the same instance whatever this says; render_lane launches shade_slim_key().
  // Volume renders (PlanInputs::volumes): k_volume runs between extend and shade of every bounce, k_shadow_volume ahead
  // of k_shadow where the shadow stage runs; `shade` then names a KF_SHADE_VOL instance. none = not launched.
  bool volumes = false;
  InstanceKey volume_key, shadow_volume_key;
  // Textured renders (PlanInputs::faces): `extend` names a KF_EXTEND_FACES instance, `shade` a KF_SHADE_FACES one.
  bool faces = false;
  // Camera rays traced where they are made (kernels/pathtrace.hip, k_camera): one launch generates, culls and traces the
  // batch's camera rays, one ray per lane, and writes their hit records; the first extend is the k_extend_deferred
  // instance over the few rays k_camera could not finish. `extend` names the same instance whatever this says.
  // camera_mode: k_camera's test argument — bit 0 every surviving ray defers, bits 8.. a stack limit below kCamStack.
  bool camera_trace = false;
  uint32_t camera_mode = 0;
  InstanceKey extend_deferred_key() const {
    InstanceKey k = camera_trace ? extend : InstanceKey{};
    if (camera_trace) k.family = KF_EXTEND_DEFERRED;
    return k;
  }
  bool slim_state = false;
  InstanceKey shade_slim_key() const {
    InstanceKey k = slim_state ? shade_early : InstanceKey{};
    if (slim_state) k.arg[1] = 1;
    return k;
  }
  // The first vertex shaded in the lane that traced the camera ray (kernels/pathtrace.hip, k_camera_vertex): the camera
  // launch is k_camera_vertex<shade_early's table>, the first extend the ordinary `extend` instance over the rays that
  // launch deferred, the first shade `shade_early` (or its slim instance) in append mode. Every field above keeps its value.
  bool camera_vertex = false;
  // The camera launch (k_camera or k_camera_vertex) is the instance whose sample loop reads the per-pixel table and
  // steps a sample cursor (kernels/camera_pixel.hip.h). Every field above keeps its value.
  bool pixel_table = false;
  // The camera launch's cull reads the root from the staged window (k_camera / k_camera_vertex, ROOT_LDS): only where
  // the root is node 0, the first node stage_nodes copies.
  bool cull_root_lds = false;
  // The camera launch's instance: k_camera_vertex<shade_early's DRV, TABLE, ROOT_LDS> or k_camera<TABLE, ROOT_LDS>;
  // none: the batch starts with k_generate.
  InstanceKey camera_key() const {
    InstanceKey k;
    if (camera_vertex) {
      k.family = KF_CAMERA_VERTEX;
      k.arg[0] = shade_early.arg[0]; k.arg[1] = pixel_table; k.arg[2] = cull_root_lds;
    } else if (camera_trace) {
      k.family = KF_CAMERA;
      k.arg[0] = pixel_table; k.arg[1] = cull_root_lds;
    }
    return k;
  }
};
// The EngineSelect a traversal instance of width w amounts to on this image (0 = three waves, 1 = four, the flat engine
// copy only, 2 = four, the direct copy only) — run_traversal picks the three-wave kernels' copy from the image.
inline EngineSelect engine_of_width(const EngineSelect &e, const DevScene &s, int w) {
  EngineSelect l = e;
  l.wide = w != 0;
  l.wide_direct = w == 2;
  l.direct = w != 1 && CRT_DIRECT_LEAVES != 0 && s.direct_leaves != 0;
  return l;
}
// CRT_OK and the plan, or CRT_ERR_UNSUPPORTED and a plan that names nothing: a launch the image cannot take is refused,
// never made. engine_accepts is asked once per traversal-bearing instance the plan names, with the EngineSelect that
// instance amounts to and its own cold argument.
inline int plan_launches(const PlanInputs &q, LaunchPlan &out) {
  const EngineSelect &e = q.engine;
  LaunchPlan pl;
  pl.fused = q.force_fused >= 0 ? q.force_fused != 0 : !(q.prefer_stage && q.total >= q.stage_min_paths);
  // the stats build is the per-stage one; no fused instance carries the lights at infinity (see k_path) — nor a tail then
  if (q.stats || q.has_inf_lights) pl.fused = false;
  // Volume renders: always one launch per stage — no fused instance and no tail carries the walk (the general shade
  // instances sit at their register limit, below; the walk is a kernel of its own between two stages).
  if (q.volumes) pl.fused = false;
  pl.volumes = q.volumes;
  if (q.faces) pl.fused = false;  // textured renders likewise: the FACES instances are per-stage kernels
  pl.faces = q.faces;
  const bool stage = !pl.fused, lit = q.n_lights > 0;
  pl.wide = stage && e.wide;  // the fused kernel is a three-wave kernel whatever the scene prefers
  // The TAIL: from bounce `tail_from` on, what is left of the batch — roulette has ended all but a few paths per ten
  // thousand by then (bench: 6.6 M of 531 M rays at bounce 4, 0.1 M at bounce 6) — runs as ONE launch of the fused
  // path-loop kernel over the same segments instead of two or three launches per bounce up to the depth limit (bench,
  // depth 32: 52 launches, ~2 ms of a 137 ms step). Not for the stats build: its kernels count.
  const bool tail = stage && q.tail_from > 0 && !q.stats && !q.has_inf_lights && !q.volumes && !q.faces;
  if (tail) pl.tail_at = (uint32_t)q.tail_from;
  // camera paths as 16-byte records: per-stage launches of an UNLIT scene, pinhole camera, static scene
  // (not in a volume render: k_volume reads and rewrites the full form)
  pl.cam_compact = (q.cam_compact_build && stage && q.cam_compact_ok && !lit && !q.lens && !q.has_motion && !q.volumes && !q.faces) ? 1u : 0u;
  // The root cull (generate_segment_cull): per-stage launches of an image whose root is a node, when a camera ray that
  // escapes ends on the sky gradient — a depth limit above 0 and no light at infinity (their escaped rays take the
  // vertex step) — and where the frame shows enough background for it to pay (CRT_ROOT_CULL=1 skips that estimate). Not
  // in the stats build: its kernels count the node visits the oracle counts. Lens cameras, moving instances, adaptive
  // stopping and curve images qualify: the root step depends on none of them. The compact form then carries plane d
  // (cam_compact == 2) where the shade instances hold that form: simple-material tables. The general instances sit at
  // their register limit (k_shade<2, false, false, false, false> gained three spilled registers with it) and read the
  // full form instead.
  pl.root_cull = q.root_cull_build && q.root_cull_knob != 0 && (q.root_cull_knob > 0 || q.root_miss_share >= kRootCullMinShare) &&
                 stage && !q.stats && q.scene.root != CRT_INVALID_ID && q.max_depth > 0 && !q.has_inf_lights &&
                 !q.volumes;  // a ray that misses the root's boxes may still cross a region
  if (pl.root_cull && pl.cam_compact) pl.cam_compact = q.mats_kind == 0 ? 2u : 0u;
  pl.shadow = stage && lit && q.strategy != CRT_STRATEGY_BSDF;
  pl.noclassify_from = q.noclassify_from;
  // The cold per-ray state the image can need (DevScene::cold) picks the closest-hit kernels' instance: none / the
  // pending normal only / everything for k_extend, none / everything for the k_path of simple-material tables; general
  // tables run the full-cold k_path, or its packet-free instance; a curve image one instance each: everything + the
  // arm(s). The stats build counts on the full-cold instances.
  const int curve_cold = e.curve ? (int)kColdAll | e.curve_cold() : 0;
  const bool simple = q.mats_kind == 0, drv = simple && q.mat_derived;
  pl.ext_cold = e.curve ? curve_cold : (q.stats ? (int)kColdAll : e.ext_cold);
  pl.path_cold = e.curve ? curve_cold : (simple ? (e.path_cold & (int)kColdAll) : (int)kColdAll | (q.nopk_build ? e.path_cold & (int)kNoPackets : 0));
  auto key = [](KernelFamily f, int a0, int a1 = 0, int a2 = 0, int a3 = 0, int a4 = 0) {
    InstanceKey k;
    k.family = f;
    k.arg[0] = (uint8_t)a0; k.arg[1] = (uint8_t)a1; k.arg[2] = (uint8_t)a2; k.arg[3] = (uint8_t)a3; k.arg[4] = (uint8_t)a4;
    return k;
  };
  // the per-stage traversal kernels' width: curve images run three-wave instances only, and the stats build of a
  // direct-leaf image counts on them too (the counters do not depend on the engine split)
  const bool wdirect = pl.wide && e.wide_direct && q.wide_direct_build;
  const int width = e.curve ? 0 : (wdirect ? (q.stats ? 0 : 2) : (pl.wide ? 1 : 0));
  int shadow_cold = (int)kColdAll;  // an any-hit query keeps no cold state: k_shadow serves every image without curves
  if (pl.fused || tail)  // simple-material tables: derived records or raw ones, cold none / everything
    pl.path = key(KF_PATH, q.mats_kind, lit, simple && pl.path_cold != 0 ? (int)kColdAll : pl.path_cold, drv);
  if (stage) {
    pl.extend = key(KF_EXTEND, q.stats, width, pl.ext_cold);
    // the shade instance: material table, lights at infinity, four waves (simple materials without lights at infinity,
    // when the scene runs the wide kernels), whether the light list is empty; a mapped dome: the instances with its arm
    const bool shade_wide = simple && !q.has_inf_lights && pl.wide && !q.mat_index && q.shade_wide != 0;
    pl.shade = q.has_env ? key(KF_SHADE_ENV, q.mats_kind, drv) : key(KF_SHADE, q.mats_kind, q.has_inf_lights, shade_wide, lit, drv);
    if (q.volumes) {  // the VOL instances: three waves, raw records; neither the pipelined kernel nor the slim state
      pl.shade = key(KF_SHADE_VOL, q.mats_kind, q.has_env ? 2 : (q.has_inf_lights ? 1 : 0), lit);
      pl.volume_key = key(KF_VOLUME, 0);
      if (pl.shadow) pl.shadow_volume_key = key(KF_SHADOW_VOLUME, 0);
    } else if (q.faces) {  // the FACES instances: the engine width as picked, the cold state with u, v; three-wave shade, raw records
      const int faces_cold = e.curve ? curve_cold : (int)kColdAll;
      pl.ext_cold = faces_cold;
      pl.extend = key(KF_EXTEND_FACES, width, faces_cold);
      pl.shade = key(KF_SHADE_FACES, q.mats_kind, q.has_env ? 2 : (q.has_inf_lights ? 1 : 0), lit);
    } else if (shade_wide && shade_pipe_fits(q) && q.noclassify_from > 0) pl.shade_early = key(KF_SHADE_PIPE, drv);
    pl.slim_state = pl.shade_piped() && q.no_emitter && q.slim_state != 0;
    if (pl.shadow) {
      if (e.curve) { pl.shadow_key = key(e.cubic ? KF_SHADOW_CUBIC : KF_SHADOW_CURVE, q.stats); shadow_cold = curve_cold; }
      else pl.shadow_key = key(KF_SHADOW, q.stats, width);
    }
    // k_camera: the per-stage pipeline with camera paths in the compact form (so: unlit, pinhole, static, no volumes), on
    // the flat four-wave engine without cold state — the one instance k_extend_deferred is built for — of an image with
    // packets whose root is a node, a depth limit of at least one bounce, every pixel sampling. Not the stats build: its
    // kernels count the steps of every ray. With or without the root cull.
    pl.camera_trace = q.camera_trace_build && q.camera_trace_knob != 0 && !q.stats && !q.volumes && !q.partial_active &&
                      pl.cam_compact != 0 && width == 1 && pl.ext_cold == 0 && q.max_depth >= 1 && q.scene.root != CRT_INVALID_ID &&
                      q.scene.n_packets > 0 && q.scene.has_packets != 0 && q.scene.direct_leaves == 0 &&
                      (q.camera_trace_knob > 0 || q.scene.n_nodes <= kCameraTraceMaxNodes);
    if (pl.camera_trace) pl.camera_mode = q.camera_trace_knob == 2 ? 1u : (q.camera_trace_knob == 3 ? (1u << 8) : 0u);
    // k_camera_vertex: k_camera's batches whose first shade is the pipelined instance (unlit, simple materials, the whole
    // table in LDS: the vertex function the two kernels share) and has a vertex to shade — a depth limit of at least 1.
    pl.camera_vertex = pl.camera_trace && pl.shade_piped() && q.max_depth >= 1 && q.camera_vertex_knob != 0;
    // the per-pixel table: either camera launch (both run static pinhole batches over every owned pixel), where the
    // renderer holds one
    pl.pixel_table = pl.camera_trace && q.pixel_table_knob != 0 && q.pixel_table_ready;
    pl.cull_root_lds = pl.camera_trace && pl.root_cull && q.cull_root_lds_knob != 0 && q.scene.root == 0 && q.scene.n_nodes > 0;
  }
  const bool ok = !(q.volumes && q.stats) &&  // the stats build counts no walk: refused (crt_render_samples_stats)
                  !(q.faces && (q.stats || q.volumes)) &&  // textured renders: no stats build, not beside volumes
                  !(q.faces && pl.extend.arg[0] == 2 && !q.wide_direct_build) &&
                  (pl.path.none() || engine_accepts(engine_of_width(e, q.scene, 0), q.scene, pl.path.arg[2])) &&
                  (pl.extend.none() || engine_accepts(engine_of_width(e, q.scene, width), q.scene, pl.faces ? pl.extend.arg[1] : pl.extend.arg[2])) &&
                  (pl.shadow_key.none() || engine_accepts(engine_of_width(e, q.scene, width), q.scene, shadow_cold));
  if (!ok) { pl.path = pl.extend = pl.shade = pl.shade_early = pl.shadow_key = pl.volume_key = pl.shadow_volume_key = InstanceKey{}; pl.slim_state = false; pl.faces = false; pl.camera_trace = false; pl.camera_mode = 0; pl.camera_vertex = false; pl.pixel_table = false; pl.cull_root_lds = false; }
  out = pl;
  return ok ? CRT_OK : CRT_ERR_UNSUPPORTED;
}

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
