// Which traversal engine and which kernel instances run (not part of the ABI): the engine-split build switches,
// select_engine and the renderer's launch plan (plan_launches) with the instance lists it names. Plain C++17 over the
// device image format: no host type and no HIP header, so the host, the kernels and the CPU sweeps under
// tests/launch_plan/ all compile this file as it stands.
#pragma once

#include "dev_image.h"
#include "../../include/crt.h"

namespace crt {

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
// The four-wave arena's split, by tree and by kernel (kernels/traverse_pool.hip.h, "Round 4", has the measurements): one
// stack entry more on a large tree or an instance-heavy scene, which gives up most of the node window for it, and one
// more in the kernels whose rays all carry one mask (umask: no mask plane). The one statement of it: run_traversal splits
// its arena with these two functions and select_engine reports them.
CRT_HOST_DEVICE constexpr int wide_stack(bool deep_tree, bool umask) { return CRT_POOL_STACK_WIDE + (deep_tree ? 1 : 0) + (umask ? 1 : 0); }
CRT_HOST_DEVICE constexpr int wide_nodes(bool deep_tree) { return deep_tree ? CRT_POOL_NODES_WIDE_DEEP : CRT_POOL_NODES_WIDE; }

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
  // umask = true whatever `renderer` says: the report keeps the renderer's figure for the batched queries too
  e.lds_stack = e.wide ? (uint32_t)wide_stack(deep, true) : (deep ? (uint32_t)CRT_POOL_STACK_DEEP : (uint32_t)CRT_POOL_STACK);
  e.window = e.wide ? (uint32_t)wide_nodes(deep) : (deep ? (uint32_t)CRT_POOL_NODES_DEEP : (uint32_t)CRT_POOL_NODES);
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
                               KF_EXTEND_FACES, KF_SHADE_FACES, KF_SHADE_GUIDED };
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
// Guided renders (PlanInputs::guided, crt_renderer_set_guiding). k_shade_guided<MATS, INF, LIT>: the shade instances whose
// secondary vertices bounce through the guiding field and weigh NEE against the mixture pdf, instantiated like
// k_shade_vol's — three waves, raw material records. A list of its own: a plan names them in `shade` with this family;
// extend and shadow are the unbound plan's instances.
#define CRT_INSTANCES_SHADE_GUIDED(X) /* k_shade_guided<MATS, INF, LIT> */ \
  X(SHADE_GUIDED, k_shade_guided, 0, 0, false) X(SHADE_GUIDED, k_shade_guided, 0, 0, true) X(SHADE_GUIDED, k_shade_guided, 0, 1, true) X(SHADE_GUIDED, k_shade_guided, 0, 2, true) \
  X(SHADE_GUIDED, k_shade_guided, 1, 0, false) X(SHADE_GUIDED, k_shade_guided, 1, 0, true) X(SHADE_GUIDED, k_shade_guided, 1, 1, true) X(SHADE_GUIDED, k_shade_guided, 1, 2, true) \
  X(SHADE_GUIDED, k_shade_guided, 2, 0, false) X(SHADE_GUIDED, k_shade_guided, 2, 0, true) X(SHADE_GUIDED, k_shade_guided, 2, 1, true) X(SHADE_GUIDED, k_shade_guided, 2, 2, true)
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
  // A guiding field is bound (crt_renderer_set_guiding): one launch per stage whatever the batch size, the GUIDED shade
  // instances; extend and shadow as unbound. No fused kernel and no tail, no compact camera paths, no camera-trace /
  // camera-vertex / pixel-table launch, no pipelined or slim shade, no derived material table. Lanes stay. Not in the
  // stats build, not with volumes or textures: refused. false: exactly the plan of a renderer that never heard of it.
  bool guided = false;
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
  // Guided renders (PlanInputs::guided): `shade` names a KF_SHADE_GUIDED instance.
  bool guided = false;
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
  if (q.guided) pl.fused = false;  // guided renders likewise: the GUIDED instances are per-stage kernels
  pl.guided = q.guided;
  const bool stage = !pl.fused, lit = q.n_lights > 0;
  pl.wide = stage && e.wide;  // the fused kernel is a three-wave kernel whatever the scene prefers
  // The TAIL: from bounce `tail_from` on, what is left of the batch — roulette has ended all but a few paths per ten
  // thousand by then (bench: 6.6 M of 531 M rays at bounce 4, 0.1 M at bounce 6) — runs as ONE launch of the fused
  // path-loop kernel over the same segments instead of two or three launches per bounce up to the depth limit (bench,
  // depth 32: 52 launches, ~2 ms of a 137 ms step). Not for the stats build: its kernels count.
  const bool tail = stage && q.tail_from > 0 && !q.stats && !q.has_inf_lights && !q.volumes && !q.faces && !q.guided;
  if (tail) pl.tail_at = (uint32_t)q.tail_from;
  // camera paths as 16-byte records: per-stage launches of an UNLIT scene, pinhole camera, static scene
  // (not in a volume render: k_volume reads and rewrites the full form)
  pl.cam_compact = (q.cam_compact_build && stage && q.cam_compact_ok && !lit && !q.lens && !q.has_motion && !q.volumes && !q.faces && !q.guided) ? 1u : 0u;
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
    } else if (q.guided) {  // the GUIDED instances: three-wave shade, raw records; extend and shadow as they are
      pl.shade = key(KF_SHADE_GUIDED, q.mats_kind, q.has_env ? 2 : (q.has_inf_lights ? 1 : 0), lit);
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
                  !(q.guided && (q.stats || q.volumes || q.faces)) &&  // guided renders: no stats build, neither volumes nor textures
                  (pl.path.none() || engine_accepts(engine_of_width(e, q.scene, 0), q.scene, pl.path.arg[2])) &&
                  (pl.extend.none() || engine_accepts(engine_of_width(e, q.scene, width), q.scene, pl.faces ? pl.extend.arg[1] : pl.extend.arg[2])) &&
                  (pl.shadow_key.none() || engine_accepts(engine_of_width(e, q.scene, width), q.scene, shadow_cold));
  if (!ok) { pl.path = pl.extend = pl.shade = pl.shade_early = pl.shadow_key = pl.volume_key = pl.shadow_volume_key = InstanceKey{}; pl.slim_state = false; pl.faces = false; pl.guided = false; pl.camera_trace = false; pl.camera_mode = 0; pl.camera_vertex = false; pl.pixel_table = false; pl.cull_root_lds = false; }
  out = pl;
  return ok ? CRT_OK : CRT_ERR_UNSUPPORTED;
}

}  // namespace crt
