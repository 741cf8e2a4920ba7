// What the CPU sweeps of the launch plan share (tests/launch_plan/*.cpp): REQUIRE, the plan comparisons, and the input
// grid of plan_sweep.cpp with its case fields. Plain C++17 against crust-render_amd/csrc/launch_plan.h alone — the one
// project header a sweep program sees.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../crust-render_amd/csrc/launch_plan.h"

#ifndef CRT_CAM_COMPACT_BUILD
#define CRT_CAM_COMPACT_BUILD 1
#endif

using namespace crt;

constexpr int kPipeMatMaxForTests = 40;  // the value handed to the planner as pipe_mat_max (any positive number serves)

// One case: the facts of an image and a renderer, as small integers (the columns of the decision table).
enum Field { F_DIRECT, F_PACKETS, F_POOL_STACK, F_NODES, F_COLD, F_ROOT_VALID, F_WANT_WIDE, F_MATS, F_LIGHTS, F_STRATEGY, F_DERIVED,
             F_STATS, F_FORCE_FUSED, F_BIG_BATCH, F_TAIL_FROM, F_MAX_DEPTH, F_NOCLASSIFY_FROM, F_SHADE_WIDE, F_SHADE_PIPE, F_MAT_INDEX,
             F_PARTITION, F_MOTION, F_LENS, F_CAM_COMPACT_OK, F_ROOT_CULL_KNOB, F_MISS_SHARE_HIGH, F_MATS_OVER, kRowFields };

// The case a violated REQUIRE reports: the integer row the grid is at (sweep_grid sets it before every check), or, in
// the programs with a grid of their own, the text they format into g_case.
inline const int *g_row = nullptr;
inline char g_case[640] = "";
[[noreturn]] inline void violated(const char *cond, int line) {
  fprintf(stderr, "violated: %s (line %d)\n  case:", cond, line);
  if (g_row) for (int k = 0; k < kRowFields; k++) fprintf(stderr, " %d", g_row[k]);
  else fprintf(stderr, " %s", g_case);
  fprintf(stderr, "\n");
  exit(1);
}
#define REQUIRE(cond)                         \
  do {                                        \
    if (!(cond)) violated(#cond, __LINE__);   \
  } while (0)

// "The knob changes nothing the plan held before": one comparison per generation of the plan, each the one before and
// the fields the next feature added. A sweep names the generation that ends where its own feature begins.
inline bool same_before_slim(const LaunchPlan &a, const LaunchPlan &b) {  // every field the plan had before the slim form existed
  return a.fused == b.fused && a.wide == b.wide && a.tail_at == b.tail_at && a.cam_compact == b.cam_compact && a.root_cull == b.root_cull &&
         a.shadow == b.shadow && a.noclassify_from == b.noclassify_from && a.ext_cold == b.ext_cold && a.path_cold == b.path_cold &&
         a.path == b.path && a.extend == b.extend && a.shade == b.shade && a.shade_early == b.shade_early && a.shadow_key == b.shadow_key;
}
inline bool same_before_camera_trace(const LaunchPlan &a, const LaunchPlan &b) {  // ... before the camera trace: the slim form, volumes
  return same_before_slim(a, b) && a.volumes == b.volumes && a.volume_key == b.volume_key && a.shadow_volume_key == b.shadow_volume_key &&
         a.slim_state == b.slim_state && a.shade_slim_key() == b.shade_slim_key();
}
inline bool same_before_camera_vertex(const LaunchPlan &a, const LaunchPlan &b) {  // ... before the camera vertex: the camera trace
  return same_before_camera_trace(a, b) && a.camera_trace == b.camera_trace && a.camera_mode == b.camera_mode &&
         a.extend_deferred_key() == b.extend_deferred_key();
}
inline bool same_before_pixel_table(const LaunchPlan &a, const LaunchPlan &b) {  // ... before the per-pixel table: the camera vertex
  return same_before_camera_vertex(a, b) && a.camera_vertex == b.camera_vertex;
}

inline DevScene scene_of(const int *v) {
  DevScene s{};
  s.direct_leaves = (uint32_t)v[F_DIRECT]; s.n_packets = (uint32_t)v[F_PACKETS]; s.has_packets = v[F_PACKETS] != 0;
  s.pool_stack = (uint32_t)v[F_POOL_STACK]; s.n_nodes = (uint32_t)v[F_NODES]; s.cold = (uint32_t)v[F_COLD];
  s.root = v[F_ROOT_VALID] ? 0u : CRT_INVALID_ID;
  return s;
}
// F_LIGHTS: 0 none, 1 finite only, 2 one at infinity, 3 a mapped dome
inline PlanInputs inputs_of(const int *v, const DevScene &s, const EngineSelect &e) {
  PlanInputs q;
  q.engine = e; q.scene = s;
  q.mats_kind = v[F_MATS]; q.mat_derived = v[F_DERIVED] != 0;
  q.n_lights = v[F_LIGHTS] ? 2u : 0u; q.has_inf_lights = v[F_LIGHTS] >= 2; q.has_env = v[F_LIGHTS] == 3;
  q.strategy = (uint32_t)v[F_STRATEGY];
  q.has_motion = v[F_MOTION] != 0; q.lens = v[F_LENS] != 0; q.mat_index = v[F_MAT_INDEX] != 0;
  q.partition = (uint32_t)v[F_PARTITION]; q.class_stats = 0;
  q.n_materials = (uint32_t)(kPipeMatMaxForTests + (v[F_MATS_OVER] ? 1 : 0)); q.max_depth = (uint32_t)v[F_MAX_DEPTH];
  q.force_fused = v[F_FORCE_FUSED]; q.prefer_stage = true; q.stage_min_paths = 1000;
  q.tail_from = v[F_TAIL_FROM]; q.noclassify_from = v[F_NOCLASSIFY_FROM]; q.shade_wide = v[F_SHADE_WIDE]; q.shade_pipe = v[F_SHADE_PIPE];
  q.cam_compact_ok = v[F_CAM_COMPACT_OK] != 0; q.root_cull_knob = v[F_ROOT_CULL_KNOB];
  q.root_miss_share = v[F_MISS_SHARE_HIGH] ? 0.25f : 0.0625f;  // either side of one eighth
  q.total = v[F_BIG_BATCH] ? 2000 : 500; q.stats = v[F_STATS] != 0;
  q.cam_compact_build = CRT_CAM_COMPACT_BUILD != 0; q.wide_direct_build = CRT_WIDE_DIRECT_BUILD != 0; q.nopk_build = CRT_NOPK_BUILD != 0;
  q.shade_pipe_build = true; q.root_cull_build = true; q.pipe_mat_max = kPipeMatMaxForTests;
  return q;
}

// The grid. The scene axes reach the planner only through select_engine's outcome and four DevScene fields, so each
// distinct (EngineSelect, direct_leaves, n_packets, cold, root) is planned once. The full cross product of the remaining
// axes is 10^9 cases per engine outcome; the sweep crosses the axes that choose the pipeline and the instances (CORE)
// fully, and each group of switches that gate one form fully WITHIN the group and against CORE, the other groups at
// their defaults: every value of every axis meets every combination of the axes it is read together with.
// `check` is called once per case as check(row, scene, engine), with g_row at the row.
struct GridCounts { unsigned long long scenes = 0, noengine = 0; size_t engines = 0; };
template <class Check>
inline GridCounts sweep_grid(Check check) {
  const int colds[] = {0, 1, 2, 3, 4, 7, 2 | 16, 7 | 16, 7 | 16 | 32};
  const int nodes[] = {100, 1500, 5000};
  struct Seen { DevScene s; EngineSelect e; };
  std::vector<Seen> engines;
  GridCounts counts;
  for (int direct = 0; direct < 2; direct++) for (int packets = 0; packets <= 5; packets += 5) for (int stack = 6; stack <= 10; stack += 4)
  for (int nd : nodes) for (int cold : colds) for (int root = 0; root < 2; root++) for (int want = -1; want <= 2; want++) {
    int v[kRowFields] = {};
    v[F_DIRECT] = direct; v[F_PACKETS] = packets; v[F_POOL_STACK] = stack; v[F_NODES] = nd; v[F_COLD] = cold; v[F_ROOT_VALID] = root;
    const DevScene s = scene_of(v);
    EngineSelect e;
    counts.scenes++;
    if (select_engine(s, want, e, true) != CRT_OK) { counts.noengine++; continue; }
    bool seen = false;
    for (const Seen &o : engines)
      seen = seen || (o.s.direct_leaves == s.direct_leaves && o.s.n_packets == s.n_packets && o.s.cold == s.cold && o.s.root == s.root &&
                      o.e.wide == e.wide && o.e.wide_direct == e.wide_direct && o.e.direct == e.direct && o.e.ext_cold == e.ext_cold &&
                      o.e.path_cold == e.path_cold && o.e.curve == e.curve && o.e.cubic == e.cubic);
    if (!seen) engines.push_back({s, e});
  }
  counts.engines = engines.size();
  const int tails[] = {0, 3, 12}, depths[] = {0, 2, 32}, ncfs[] = {1, 1 << 30};
  for (const Seen &en : engines) {
    int v[kRowFields] = {};
    g_row = v;
    v[F_DIRECT] = (int)en.s.direct_leaves; v[F_PACKETS] = (int)en.s.n_packets; v[F_COLD] = (int)en.s.cold; v[F_ROOT_VALID] = en.s.root != CRT_INVALID_ID;
    // CORE: material table x lights x derived x stats x CRT_FUSED x batch size
    for (int mats = 0; mats < 3; mats++) for (int lights = 0; lights < 4; lights++) for (int drv = 0; drv < 2; drv++)
    for (int stats = 0; stats < 2; stats++) for (int ff = -1; ff <= 1; ff++) for (int big = 0; big < 2; big++) {
      auto defaults = [&] {
        v[F_MATS] = mats; v[F_LIGHTS] = lights; v[F_DERIVED] = drv; v[F_STATS] = stats; v[F_FORCE_FUSED] = ff; v[F_BIG_BATCH] = big;
        v[F_STRATEGY] = CRT_STRATEGY_POWER; v[F_TAIL_FROM] = 12; v[F_MAX_DEPTH] = 32; v[F_NOCLASSIFY_FROM] = 1 << 30; v[F_SHADE_WIDE] = -1;
        v[F_SHADE_PIPE] = 1; v[F_MAT_INDEX] = 0; v[F_PARTITION] = 0; v[F_MOTION] = 0; v[F_LENS] = 0; v[F_CAM_COMPACT_OK] = 1;
        v[F_ROOT_CULL_KNOB] = -1; v[F_MISS_SHARE_HIGH] = 1; v[F_MATS_OVER] = 0;
      };
      // the loop's shape: strategy x tail x depth x noclassify_from
      defaults();
      for (int strategy = CRT_STRATEGY_POWER; strategy <= CRT_STRATEGY_BSDF; strategy++) for (int t : tails) for (int d : depths) for (int n : ncfs) {
        v[F_STRATEGY] = strategy; v[F_TAIL_FROM] = t; v[F_MAX_DEPTH] = d; v[F_NOCLASSIFY_FROM] = n;
        check(v, en.s, en.e);
      }
      // the shade instance's gates
      defaults();
      for (int bits = 0; bits < 128; bits++) for (int t = 0; t < 2; t++) {
        v[F_SHADE_WIDE] = (bits & 1) ? 0 : -1; v[F_SHADE_PIPE] = (bits >> 1) & 1; v[F_MAT_INDEX] = (bits >> 2) & 1; v[F_PARTITION] = (bits >> 3) & 1;
        v[F_MATS_OVER] = (bits >> 4) & 1; v[F_NOCLASSIFY_FROM] = (bits & 32) ? 1 : 1 << 30; v[F_MOTION] = (bits >> 6) & 1; v[F_TAIL_FROM] = t ? 3 : 12;
        check(v, en.s, en.e);
      }
      // the camera form's and the root cull's gates
      defaults();
      for (int bits = 0; bits < 16; bits++) for (int knob = -1; knob <= 1; knob++) for (int d : depths) {
        v[F_MOTION] = bits & 1; v[F_LENS] = (bits >> 1) & 1; v[F_CAM_COMPACT_OK] = (bits >> 2) & 1; v[F_MISS_SHARE_HIGH] = (bits >> 3) & 1;
        v[F_ROOT_CULL_KNOB] = knob; v[F_MAX_DEPTH] = d;
        check(v, en.s, en.e);
      }
    }
  }
  g_row = nullptr;
  return counts;
}
