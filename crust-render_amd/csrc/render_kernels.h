// What the renderer's host side (render.cpp) and its kernels (kernels/pathtrace.hip) share: the types a launch passes,
// the constants both sides size things by, the kernel pointer types, and the three things pathtrace.hip defines for the
// host — what its headers alone know about this build (kKernelBuild), the single-form kernels (kStageKernels) and the
// resolver from a launch plan's keys to kernel pointers (resolve_kernels). Declarations only: no device function, no
// include of a kernel header.
#pragma once

#include <hip/hip_runtime.h>

#include "crt_internal.h"
#include "kernels/faces.hip.h"  // dev::FaceView, passed by value to the FACES shade instances
#include "kernels/guiding.hip.h"  // dev::GuideView, passed by value to the GUIDED shade instances

namespace crt {

namespace dev { struct DevMaterial; struct DevMedium; struct PixelRec; struct EnvSlot; }  // behind pointers only

using dev::kBlock;  // threads per workgroup of every launch (dev_image.h: the traversal library's launches share it)
constexpr uint32_t kMaxMedia =(1u << 14) - 1;  // the path state carries a 14-bit compact medium id (PathSoA::d)
constexpr int kNumberBlock = 1024;              // threads of k_number_media's one workgroup
constexpr int kClasses = 4;                     // material classes (launch_plan.h, material_class)
constexpr uint32_t kPixelTableMaxExtent = 1u << 24;  // a wider frame builds no per-pixel table: (float)px is exact below 2^24

// Path state: struct-of-arrays of 16-byte records, so each plane is read and written with one
// 16-byte-per-lane (1 KiB per wave) instruction — the widest, most efficient global access on CDNA4.
struct PathSoA {
  float4 *a;    // origin.xyz, dir.x
  float4 *b;    // dir.yz, beta.xy          beta: the running throughput (tracer.rs:1114)
  float4 *c;    // beta.z, L.xyz            L: radiance gathered so far
  uint4 *d;     // sampler pattern of the K_PATH domain | owned-pixel index |
                // n_rec (low 16) + remaining depth (high 16) | sample-in-batch (low 16) + kPrevValid + kPrevDelta
                // + carried-medium id (high 14)
  float4 *e;    // previous vertex position + previous bounce pdf (PrevBounce, tracer.rs:899-906); lit scenes only
                // A PHASE previous vertex (PrevVertex::Phase, a scatter inside a volume region: k_volume) needs no bit of
                // its own: it is kPrevValid without kPrevDelta with e = (p, phase_pdf). The emitter weights read nothing
                // else of a previous vertex — the material's eval() check of a surface one is already folded into
                // kPrevDelta (pathtrace.hip, emission_weight) — so the two kinds are one record here.
  float *time;  // shutter time; scenes with motion only
  // The SLIM form, between two launches of k_shade_pipe<DRV, true> only (LaunchPlan::slim_state: no record of the
  // material table emits, so L is +0 at every vertex; no media, so no carried medium):
  //   a, b  as above
  //   c     beta.z | sampler pattern (bits) | owned-pixel index + kPrevDelta-bit << 31 (bits) | sample-in-batch (bits)
  //   d     neither written nor read: n_rec and the remaining depth follow from the bounce number, which the launch
  //         is told, kPrevValid is "not the first bounce"
  // 48 bytes per path instead of 64. Every other consumer (k_extend reads a and b in either form; k_shade, k_path) sees
  // the full form: the launch before it is told to write that (out_full).
};
struct HitSoA { float4 *h; uint32_t *geom; };  // t, ray-facing normal; geom id | front_face << 31, ~0 = miss
struct ShadowSoA { float4 *a, *b, *c; };       // origin + tmax; dir + time; contribution + target (bits)

// Queues are segmented per workgroup: workgroup b owns slots [b * seg_cap, (b + 1) * seg_cap) of every
// state buffer and of the shadow queue, and keeps the number of live entries of its segment in seg[]. A
// workgroup compacts its own survivors with a wave ballot + popcount prefix and an LDS counter, so the
// wavefront has NO global atomics on its data path (a single returning atomic per wave on one queue head
// saturates near 88 M/s on this chip — more than the whole shade stage costs).
//
// Direction bins: a workgroup's segment of a PATH buffer is split into kBins sub-segments, one per octant of the
// ray direction, and shade appends every continuing path to the sub-segment of its new direction. The next
// extend then walks the sub-segments in turn, so the 64 rays of a wave share their direction signs (same
// near-to-far child order, similar subtrees) and come from neighbouring pixels: secondary rays regain most of
// the coherence of camera rays without a sort pass. Price: kBins x the slot index space of the path and hit
// planes (address space only — untouched slots cost neither bandwidth nor cache; HBM has 288 GB).
// Measured on cornellbox 1080p (profiles/README.md, r01c): 8 octant bins cut extend by only 3 % and cost shade
// 15 % — the divergence is between traversal PHASES, not between child orders — so the default is 1 bin.
#ifndef CRT_BINS
#define CRT_BINS 1
#endif
constexpr int kBins = CRT_BINS;
constexpr int kMaxGrid = 16384;
struct Counters {
  uint32_t err;
  uint32_t pad;
  unsigned long long stats[8];      // RayStats (stats.rs:128-147) in declaration order
  uint32_t seg[2][kMaxGrid * kBins];  // live paths of state buffer 0 / 1, per (workgroup, bin)
  uint32_t shadow[kMaxGrid];          // shadow requests per workgroup
  // crt_renderer_shade_class_stats: per material class, the wave executions of the vertex step that contained a
  // vertex of the class, and how many of their 64 lanes held one (lanes / (64 * waves) = the class's lane utilisation)
  unsigned long long cls_waves[4], cls_lanes[4];
  // k_camera: the camera rays of the segment it left to the first extend (k_extend_deferred); their slot numbers are in
  // the segment's part of the OTHER state buffer's plane `a`, which is free until the first shade writes its survivors
  uint32_t cam_defer[kMaxGrid];
};

struct Params {
  DevScene scene;
  uint32_t sample_begin;
  const CrtMaterial *materials;
  // One DevMaterial per record of `materials`: the per-material constants of the vertex code, derived once
  // (k_derive_materials). The DERIVED kernel instances stage and read this table and go back to `materials` only in the
  // arms shade.hip.h names; CRT_MAT_DERIVED=0 launches the instances that read `materials` alone.
  const dev::DevMaterial *mat_derived;
  uint32_t n_materials;
  // geom_id -> record of `materials` (and of `media`, `mat_class`), or nullptr: the table is indexed by geom_id itself.
  // World::attach binds a material per geometry (rt_world.rs:111-122) and an instanced city binds the same few looks
  // tens of thousands of times: PointInstancedMedCity has 40 008 geometry ids and 9.3 MB of records that are 133
  // distinct ones or fewer — deduplicated (crt_renderer_new) the table stages in LDS like every other scene's.
  const uint16_t *mat_index;
  const dev::DevMedium *media;        // per geom_id: the material's interior medium (present == 0: none)
  const dev::DevMedium *media_by_id;  // the present ones, by compact id - 1
  const CrtLight *lights;
  uint32_t n_lights;
  uint32_t has_inf_lights;  // any DISTANT / DOME entry: escaping rays then run escaped_emission
  CrtCamera camera;
  uint32_t width, height, max_depth;
  int32_t frame, strategy, filter_kind;
  float filter_radius;
  uint32_t has_motion;
  const uint32_t *pixel_index;  // owned pixels: j * width + i
  uint32_t n_pix;
  // Adaptive stopping (tracer.rs:609-617): the pixels still sampling. active == nullptr: all n_pix, in order.
  // A path carries its ACTIVE slot; the staging film is indexed [sample][active slot].
  const uint32_t *active;
  uint32_t n_act;
  uint32_t seg_cap;             // slots per workgroup segment
  // Material classes (shade's partition key): one byte per geom_id, and whether more than one class occurs at all —
  // a one-class scene (cornellbox, MedCity) keeps the single pending ring and pays nothing.
  const uint8_t *mat_class;
  uint32_t partition;
  uint32_t class_stats;         // count Counters::cls_* in the vertex step (diagnostic, off by default)
  // Per-stage pipeline, pinhole camera, no motion blur: a camera path is the 16 bytes (direction, sampler pattern) in
  // plane `a` — its origin is the camera's, its throughput 1, its radiance 0, pixel / sample / depth follow from the slot
  // number (generate_segment). Set per batch by Renderer::render. 2: the compact form under the root cull — the survivors
  // are compacted, so a slot no longer names its sample: plane `d` is written too and read back (compact_camera_path).
  uint32_t cam_compact;
  // Per-stage launches: generate finishes every camera ray that touches no child box of the root node on the spot — the
  // sky gradient into the staging film, the counters the miss step feeds — and appends only the others to its segment
  // (generate_segment_cull). Set per batch from the launch plan (launch_plan.h, plan_launches), which holds the rule.
  uint32_t root_cull;
  // The library's table of live environments (environment.cpp), read by the mapped-dome instances only (k_shade_env):
  // a CRT_LIGHT_DOME_MAP record names its environment by id. nullptr when the light list holds no such record.
  const dev::EnvSlot *envs;
};
struct VolArgs { const dev::VolRegionRec *regions; const float *grid; uint32_t n_regions; };
struct PixelStats { double lum_sum, lum_sq; };  // adaptive stopping: a pixel's luminance statistics (k_resolve_adaptive)

// What only the kernel headers know about this build, as values: the record sizes behind the forward declarations
// above, the material-table budgets of the LDS arenas, and the build switches that gate kernel forms.
struct KernelBuild {
  size_t sizeof_material, sizeof_medium, sizeof_pixel_rec;  // sizeof(DevMaterial), sizeof(DevMedium), sizeof(PixelRec)
  int mat_lds_max;   // material records the three-wave arena stages: mat_lds_max(kArenaDwords)
  int pipe_mat_max;  // ... and the pipelined shade kernel's arena: kPipeMatMax
  bool root_cull, shade_pipe, regen_first;  // kRootCullBuild, kShadePipeBuild, kRegenFirst
  bool cam_compact, mat_index;              // CRT_CAM_COMPACT_BUILD, CRT_MAT_INDEX_BUILD
};
extern const KernelBuild kKernelBuild;

// ---------------------------------------------------------------------------------------------
// Kernel pointer types: one per signature of the multi-form kernels (the instance table of pathtrace.hip), one per
// single-form kernel.
// ---------------------------------------------------------------------------------------------
using ExtendFn = void (*)(Params, PathSoA, HitSoA, Counters *, int, int, CrtTravStats *);
using ExtendDeferredFn = void (*)(Params, PathSoA, HitSoA, Counters *, int, int, CrtTravStats *, const uint32_t *);
using PathFn = void (*)(Params, PathSoA, PathSoA, HitSoA, ShadowSoA, Counters *, float4 *, uint32_t, uint32_t, uint32_t, int);
using ShadeFn = void (*)(Params, PathSoA, PathSoA, HitSoA, ShadowSoA, Counters *, int, float4 *, int);
using ShadePipeFn = void (*)(Params, PathSoA, PathSoA, HitSoA, Counters *, int, float4 *, int, uint32_t, int);
using CameraVertexFn = void (*)(Params, PathSoA, PathSoA, Counters *, uint32_t, uint32_t, float4 *, uint32_t, int, const dev::PixelRec *);
using CameraFn = void (*)(Params, PathSoA, uint32_t *, HitSoA, Counters *, uint32_t, uint32_t, float4 *, uint32_t, const dev::PixelRec *);
using ShadowFn = void (*)(Params, PathSoA, ShadowSoA, Counters *, float4 *, CrtTravStats *);
using ShadeVolFn = void (*)(Params, PathSoA, PathSoA, HitSoA, ShadowSoA, Counters *, int, float4 *, int, uint32_t *);
// Textured renders: the hit's (prim_id, u, v, 0) record plane beside HitSoA — an argument of its own, so that no other
// kernel's arguments change — and the aggregate's tables (kernels/faces.hip.h).
using ExtendFacesFn = void (*)(Params, PathSoA, HitSoA, Counters *, int, int, CrtTravStats *, uint4 *);
using ShadeFacesFn = void (*)(Params, PathSoA, PathSoA, HitSoA, ShadowSoA, Counters *, int, float4 *, int, dev::FaceView, const uint4 *);
// Guided renders: the field's view (kernels/guiding.hip.h) — an argument of its own, as above.
using ShadeGuidedFn = void (*)(Params, PathSoA, PathSoA, HitSoA, ShadowSoA, Counters *, int, float4 *, int, dev::GuideView);

using GenerateFn = void (*)(Params, PathSoA, Counters *, uint32_t, uint32_t, float4 *);
using VolumeFn = void (*)(Params, PathSoA, HitSoA, Counters *, int, int, VolArgs);
using ShadowVolumeFn = void (*)(Params, ShadowSoA, const uint32_t *, Counters *, VolArgs);
using ResolveFn = void (*)(const float4 *, uint32_t, uint32_t, float4 *);
using ResolveAdaptiveFn = void (*)(const float4 *, const uint32_t *, uint32_t, uint32_t, float4 *, PixelStats *, uint32_t *, uint32_t, float);
using CompactActiveFn = void (*)(const uint32_t *, uint32_t, uint32_t *, uint32_t *);
using FilmOutFn = void (*)(const float4 *, uint32_t, float *);
using FillPixelTableFn = void (*)(const uint32_t *, uint32_t, uint32_t, int, dev::PixelRec *);
using DeriveMaterialsFn = void (*)(const CrtMaterial *, uint32_t, dev::DevMaterial *);
using BuildMediaFn = void (*)(const CrtMaterial *, uint32_t, dev::DevMedium *);
using NumberMediaFn = void (*)(uint32_t, dev::DevMedium *, dev::DevMedium *, uint32_t *);

// The single-form kernels, filled once in pathtrace.hip.
struct StageKernels {
  GenerateFn generate;
  VolumeFn volume;
  ShadowVolumeFn shadow_volume;
  ResolveFn resolve;
  ResolveAdaptiveFn resolve_adaptive;
  CompactActiveFn compact_active;
  FilmOutFn film_out;
  FillPixelTableFn fill_pixel_table;
  DeriveMaterialsFn derive_materials;
  BuildMediaFn build_media;
  NumberMediaFn number_media;
};
extern const StageKernels kStageKernels;

// Every kernel one lane's batch launches through the instance table, resolved from the plan's keys; nullptr: the plan
// does not launch it.
struct BatchKernels {
  PathFn path;
  ExtendFn extend;
  ExtendDeferredFn extend_deferred;
  ShadeFn shade;
  ShadePipeFn shade_pipe, shade_slim;
  ShadeVolFn shade_vol;
  ExtendFacesFn extend_faces;     // textured renders (LaunchPlan::faces): these two in the place of extend / shade
  ShadeFacesFn shade_faces;
  ShadeGuidedFn shade_guided;     // guided renders (LaunchPlan::guided): in the place of shade
  ShadowFn shadow;
  CameraFn camera;                // the camera launch: one of the two, or neither (k_generate)
  CameraVertexFn camera_vertex;
};
// CRT_OK and the pointers — or CRT_ERR_UNSUPPORTED: a key without a row in this build (the reason in crt_last_error),
// or a plan whose keys contradict each other. Nothing is launched then.
int resolve_kernels(const LaunchPlan &plan, BatchKernels &out);

}  // namespace crt
