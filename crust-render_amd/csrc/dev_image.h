// The device image format of libcrt_amd.so (not part of the ABI): the committed-tree records, the primitive and instance
// records and the DevScene view — what the host writes (scene.cpp) and the kernels read (kernels/). Shared by both sides,
// so it holds no host type and no HIP name beyond CRT_HOST_DEVICE.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/crt.h"

namespace crt {

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
// The depth word of a cubic span's tail record: the two declarations every reader of that word needs, the host (scene.cpp
// stores it; bvh_build.cpp defines the function) and the kernels' walk (traverse.hip.h clamps to the limit).
// flatness_depth (curve.rs:122-141) of a cubic span, cp = 12 floats, max_width = 2 * max(r0, r1) with the radii as
// given: l0, eps and x = SQRT_2 * 6 * l0 / (8 * eps) in f32 in the reference's order, then clamp(floor(log2(x) / 2), 0,
// 10) read exactly from x's binary exponent — no libm on the path. 0 when l0 <= 0, max_width <= 0, x is not finite or
// x < 1. The one function that computes it: commit stores it in the span's record, the kernels read it and loop.
uint32_t cubic_flatness_depth(const float cp[12], float max_width);
constexpr uint32_t kMaxCubicDepth = 10;  // curve.rs:98 MAX_RECURSION_DEPTH
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

}  // namespace crt
