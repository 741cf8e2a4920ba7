// The renderer's launch planning (crust-render_amd/csrc/crt_internal.h: select_engine, plan_launches) on the CPU, driven
// by tests/test_launch_plan.py. Plain C++17 against the header alone; built once per build-switch tuple (-DCRT_..._BUILD).
//   plan_sweep sweep          the property sweep over the input grid; prints the case counts, exit 1 on the first violation
//   plan_sweep table < rows   one decision line per input row (kRowFields integers): the parent's decision table
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../crust-render_amd/csrc/crt_internal.h"

#ifndef CRT_CAM_COMPACT_BUILD
#define CRT_CAM_COMPACT_BUILD 1
#endif

using namespace crt;

static const int kPipeMatMaxForTests = 40;  // the value handed to the planner as pipe_mat_max (any positive number serves)

// Every key this build-switch tuple holds, and its name as the kernel's template-id with numeric arguments.
struct Named { InstanceKey key; const char *kernel; int n_args; };
#define CRT_COUNT_ARGS(...) (int)(sizeof((int[]){__VA_ARGS__}) / sizeof(int))
#define CRT_NAMED(family, kernel, ...) {CRT_INSTANCE_KEY(family, kernel, __VA_ARGS__), #kernel, CRT_COUNT_ARGS(__VA_ARGS__)},
static const Named kKeys[] = {CRT_INSTANCES_EXTEND(CRT_NAMED) CRT_INSTANCES_PATH(CRT_NAMED) CRT_INSTANCES_SHADE(CRT_NAMED)
                              CRT_INSTANCES_SHADE_PIPE(CRT_NAMED) CRT_INSTANCES_SHADOW(CRT_NAMED)};
static const Named *find_key(const InstanceKey &k) {
  for (const Named &n : kKeys)
    if (n.key == k) return &n;
  return nullptr;
}
// The lists a plan names through a derived key: camera_key(), extend_deferred_key(), shade_slim_key().
static const Named kDerivedKeys[] = {CRT_INSTANCES_CAMERA(CRT_NAMED) CRT_INSTANCES_CAMERA_VERTEX(CRT_NAMED)
                                     CRT_INSTANCES_EXTEND_DEFERRED(CRT_NAMED) CRT_INSTANCES_SHADE_PIPE_SLIM(CRT_NAMED)};
static bool none_or_derived(const InstanceKey &k) {
  if (k.none()) return true;
  for (const Named &n : kDerivedKeys)
    if (n.key == k) return true;
  return false;
}
static std::string name_of(const InstanceKey &k) {
  if (k.none()) return "-";
  const Named *n = find_key(k);
  if (!n) return "?";
  std::string s = std::string(n->kernel) + "<";
  for (int a = 0; a < n->n_args; a++) s += (a ? "," : "") + std::to_string((int)k.arg[a]);
  return s + ">";
}

// One case: the facts of an image and a renderer, as small integers (the columns of the decision table).
enum Field { F_DIRECT, F_PACKETS, F_POOL_STACK, F_NODES, F_COLD, F_ROOT_VALID, F_WANT_WIDE, F_MATS, F_LIGHTS, F_STRATEGY, F_DERIVED,
             F_STATS, F_FORCE_FUSED, F_BIG_BATCH, F_TAIL_FROM, F_MAX_DEPTH, F_NOCLASSIFY_FROM, F_SHADE_WIDE, F_SHADE_PIPE, F_MAT_INDEX,
             F_PARTITION, F_MOTION, F_LENS, F_CAM_COMPACT_OK, F_ROOT_CULL_KNOB, F_MISS_SHARE_HIGH, F_MATS_OVER, kRowFields };
static DevScene scene_of(const int *v) {
  DevScene s{};
  s.direct_leaves = (uint32_t)v[F_DIRECT]; s.n_packets = (uint32_t)v[F_PACKETS]; s.has_packets = v[F_PACKETS] != 0;
  s.pool_stack = (uint32_t)v[F_POOL_STACK]; s.n_nodes = (uint32_t)v[F_NODES]; s.cold = (uint32_t)v[F_COLD];
  s.root = v[F_ROOT_VALID] ? 0u : CRT_INVALID_ID;
  return s;
}
// F_LIGHTS: 0 none, 1 finite only, 2 one at infinity, 3 a mapped dome
static PlanInputs inputs_of(const int *v, const DevScene &s, const EngineSelect &e) {
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

// What a batch launches under a plan, as render_lane's loop runs it: the decision table's columns.
struct Launches { std::string path = "-", extend = "-", shade_first = "-", shade_last = "-", shadow = "-"; int shade_switch = -1, tail = -1, bounces = 0; };
static Launches launches_of(const LaunchPlan &pl, uint32_t max_depth) {
  Launches L;
  if (pl.fused) { L.path = name_of(pl.path); return L; }
  for (uint32_t it = 0; it <= max_depth; it++) {
    if (it >= pl.tail_at) { L.tail = (int)it; L.path = name_of(pl.path); break; }
    const std::string shade = name_of(!pl.shade_early.none() && (int)it < pl.noclassify_from ? pl.shade_early : pl.shade);
    if (it == 0) L.shade_first = shade;
    else if (shade != L.shade_first && L.shade_switch < 0) L.shade_switch = (int)it;
    L.shade_last = shade;
    L.extend = name_of(pl.extend);
    L.shadow = name_of(pl.shadow_key);
    L.bounces++;
  }
  return L;
}

static int table() {
  std::vector<int> v(kRowFields);
  for (;;) {
    for (int k = 0; k < kRowFields; k++)
      if (scanf("%d", &v[k]) != 1) return k == 0 ? 0 : 1;
    const DevScene s = scene_of(v.data());
    EngineSelect e;
    if (select_engine(s, v[F_WANT_WIDE], e, true) != CRT_OK) { printf("noengine\n"); continue; }
    LaunchPlan pl;
    if (plan_launches(inputs_of(v.data(), s, e), pl) != CRT_OK) { printf("refused\n"); continue; }
    const Launches L = launches_of(pl, (uint32_t)v[F_MAX_DEPTH]);
    printf("fused=%d wide=%d compact=%u cull=%d path=%s extend=%s shade=%s shade_last=%s switch=%d shadow=%s tail=%d bounces=%d\n", (int)pl.fused,
           (int)pl.wide, pl.cam_compact, (int)pl.root_cull, L.path.c_str(), L.extend.c_str(), L.shade_first.c_str(), L.shade_last.c_str(),
           L.shade_switch, L.shadow.c_str(), L.tail, L.bounces);
  }
}

// ---------------------------------------------------------------------------------------------
// The property sweep
// ---------------------------------------------------------------------------------------------
static const int *g_case = nullptr;
#define REQUIRE(cond)                                                                   \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      fprintf(stderr, "violated: %s\n  case:", #cond);                                  \
      for (int k = 0; k < kRowFields; k++) fprintf(stderr, " %d", g_case[k]);           \
      fprintf(stderr, "\n");                                                            \
      exit(1);                                                                          \
    }                                                                                   \
  } while (0)

static unsigned long long n_cases = 0, n_planned = 0, n_refused = 0, n_refused_beyond_aggregate = 0;

// The one check the renderer made before the plan existed: engine_accepts once per batch, on the EngineSelect of the
// per-stage launches and the closest-hit kernels' cold arguments combined.
static bool aggregate_check(const PlanInputs &q, const LaunchPlan &pl) {
  EngineSelect l = q.engine;
  l.wide = pl.wide;
  l.wide_direct = pl.wide && q.engine.wide_direct;
  l.direct = (!pl.wide || l.wide_direct) && CRT_DIRECT_LEAVES != 0 && q.scene.direct_leaves != 0;
  const bool tail = pl.tail_at != 0xffffffffu;
  return engine_accepts(l, q.scene, pl.fused ? pl.path_cold : (tail ? (pl.ext_cold & pl.path_cold) : pl.ext_cold));
}

static void check_case(const int *v, const DevScene &s, const EngineSelect &e) {
  g_case = v;
  n_cases++;
  const PlanInputs q = inputs_of(v, s, e);
  LaunchPlan pl;
  const int rc = plan_launches(q, pl);
  const InstanceKey *keys[5] = {&pl.path, &pl.extend, &pl.shade, &pl.shade_early, &pl.shadow_key};
  if (rc != CRT_OK) {
    n_refused++;
    REQUIRE(rc == CRT_ERR_UNSUPPORTED);
    for (const InstanceKey *k : keys) REQUIRE(k->none());  // a refused plan names nothing
    // the per-instance check refuses beyond the aggregate one only a simple-material table on a curve image: its k_path
    // carries no curve arm (the renderer never forms that pair: crt_renderer_new gives curve images the general instances)
    if (aggregate_check(q, pl)) { n_refused_beyond_aggregate++; REQUIRE(q.mats_kind == 0 && e.curve); }
    return;
  }
  n_planned++;
  REQUIRE(aggregate_check(q, pl));
  // 1. every key is an instance of this build
  for (const InstanceKey *k : keys) REQUIRE(k->none() || find_key(*k));
  REQUIRE(none_or_derived(pl.camera_key()) && none_or_derived(pl.extend_deferred_key()) && none_or_derived(pl.shade_slim_key()));
  // 2. engine_accepts for the launched EngineSelect, per traversal instance, with the instance's own cold bits
  const int curve_bits = (int)(kColdAll | kColdCurve | kColdCubic);
  if (!pl.path.none()) REQUIRE(engine_accepts(engine_of_width(e, s, 0), s, pl.path.arg[2]));
  if (!pl.extend.none()) REQUIRE(engine_accepts(engine_of_width(e, s, pl.extend.arg[1]), s, pl.extend.arg[2]));
  if (pl.shadow_key.family == KF_SHADOW) REQUIRE(engine_accepts(engine_of_width(e, s, pl.shadow_key.arg[1]), s, (int)kColdAll));
  if (pl.shadow_key.family == KF_SHADOW_CURVE) REQUIRE(engine_accepts(engine_of_width(e, s, 0), s, (int)(kColdAll | kColdCurve)));
  if (pl.shadow_key.family == KF_SHADOW_CUBIC) REQUIRE(engine_accepts(engine_of_width(e, s, 0), s, curve_bits));
  // 3. the structural rules
  const bool tail = pl.tail_at != 0xffffffffu;
  REQUIRE(pl.fused == (pl.extend.none() && pl.shade.none()));  // fused: the path kernel and nothing else
  REQUIRE(!pl.fused || (pl.shade_early.none() && pl.shadow_key.none() && !pl.path.none() && !tail && !pl.wide && !pl.root_cull && !pl.cam_compact));
  REQUIRE(pl.path.none() == !(pl.fused || tail));
  if (q.has_inf_lights) REQUIRE(!pl.fused && !tail && pl.path.none());  // lights at infinity, mapped domes included
  if (q.has_env) REQUIRE(pl.shade.family == KF_SHADE_ENV);
  if (q.stats) {  // the stats build: per stage, no tail, no root cull, the STATS instances
    REQUIRE(!pl.fused && !tail && !pl.root_cull && pl.path.none());
    REQUIRE(pl.extend.arg[0] == 1 && (pl.shadow_key.none() || pl.shadow_key.arg[0] == 1));
  } else {
    REQUIRE(pl.extend.none() || pl.extend.arg[0] == 0);
    REQUIRE(pl.shadow_key.none() || pl.shadow_key.arg[0] == 0);
  }
  if (s.cold & kColdCurve) {  // curve and cubic images are never wide, and run the instances with the arm(s)
    REQUIRE(!pl.wide && (pl.extend.none() || pl.extend.arg[1] == 0) && pl.shadow_key.family != KF_SHADOW);
    REQUIRE(pl.shade.none() || pl.shade.family == KF_SHADE_ENV || pl.shade.arg[2] == 0);
  }
  const bool wide_direct = (!pl.extend.none() && pl.extend.arg[1] == 2) || (pl.shadow_key.family == KF_SHADOW && pl.shadow_key.arg[1] == 2);
  if (wide_direct) REQUIRE(s.direct_leaves != 0 && CRT_WIDE_DIRECT_BUILD != 0);
  if (pl.path.arg[2] & (int)kNoPackets) REQUIRE(CRT_NOPK_BUILD != 0 && s.n_packets == 0 && s.direct_leaves != 0);
  if (!pl.shade_early.none()) {  // the pipelined shade instance: only where it fits, only before noclassify_from
    REQUIRE(pl.shade_early.family == KF_SHADE_PIPE && shade_pipe_fits(q) && pl.wide && q.shade_wide != 0 && q.noclassify_from > 0);
    REQUIRE(pl.noclassify_from == q.noclassify_from && pl.shade.family == KF_SHADE && pl.shade.arg[2] == 1 && pl.shade.arg[3] == 0);
    REQUIRE(launches_of(pl, 40).shade_switch == (q.noclassify_from <= 40 && (uint32_t)q.noclassify_from < pl.tail_at ? q.noclassify_from : -1));
  }
  REQUIRE(pl.shadow == !pl.shadow_key.none());
  REQUIRE(pl.shadow == (!pl.fused && q.n_lights > 0 && q.strategy != CRT_STRATEGY_BSDF));
  if (pl.root_cull) REQUIRE(s.root != CRT_INVALID_ID && q.max_depth > 0 && q.root_cull_knob != 0);
  if (pl.cam_compact) REQUIRE(CRT_CAM_COMPACT_BUILD != 0 && q.n_lights == 0 && !q.lens && !q.has_motion && q.cam_compact_ok);
  REQUIRE(pl.cam_compact != 2 || (pl.root_cull && q.mats_kind == 0));
}

// The grid. The scene axes reach the planner only through select_engine's outcome and four DevScene fields, so each
// distinct (EngineSelect, direct_leaves, n_packets, cold, root) is planned once. The full cross product of the remaining
// axes is 10^9 cases per engine outcome; the sweep crosses the axes that choose the pipeline and the instances (CORE)
// fully, and each group of switches that gate one form fully WITHIN the group and against CORE, the other groups at
// their defaults: every value of every axis meets every combination of the axes it is read together with.
static int sweep() {
  const int colds[] = {0, 1, 2, 3, 4, 7, 2 | 16, 7 | 16, 7 | 16 | 32};
  const int nodes[] = {100, 1500, 5000};
  struct Seen { DevScene s; EngineSelect e; };
  std::vector<Seen> engines;
  unsigned long long n_scenes = 0, n_noengine = 0;
  for (int direct = 0; direct < 2; direct++) for (int packets = 0; packets <= 5; packets += 5) for (int stack = 6; stack <= 10; stack += 4)
  for (int nd : nodes) for (int cold : colds) for (int root = 0; root < 2; root++) for (int want = -1; want <= 2; want++) {
    int v[kRowFields] = {};
    v[F_DIRECT] = direct; v[F_PACKETS] = packets; v[F_POOL_STACK] = stack; v[F_NODES] = nd; v[F_COLD] = cold; v[F_ROOT_VALID] = root;
    const DevScene s = scene_of(v);
    EngineSelect e;
    n_scenes++;
    if (select_engine(s, want, e, true) != CRT_OK) { n_noengine++; continue; }
    bool seen = false;
    for (const Seen &o : engines)
      seen = seen || (o.s.direct_leaves == s.direct_leaves && o.s.n_packets == s.n_packets && o.s.cold == s.cold && o.s.root == s.root &&
                      o.e.wide == e.wide && o.e.wide_direct == e.wide_direct && o.e.direct == e.direct && o.e.ext_cold == e.ext_cold &&
                      o.e.path_cold == e.path_cold && o.e.curve == e.curve && o.e.cubic == e.cubic);
    if (!seen) engines.push_back({s, e});
  }
  const int tails[] = {0, 3, 12}, depths[] = {0, 2, 32}, ncfs[] = {1, 1 << 30};
  for (const Seen &en : engines) {
    int v[kRowFields] = {};
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
        check_case(v, en.s, en.e);
      }
      // the shade instance's gates
      defaults();
      for (int bits = 0; bits < 128; bits++) for (int t = 0; t < 2; t++) {
        v[F_SHADE_WIDE] = (bits & 1) ? 0 : -1; v[F_SHADE_PIPE] = (bits >> 1) & 1; v[F_MAT_INDEX] = (bits >> 2) & 1; v[F_PARTITION] = (bits >> 3) & 1;
        v[F_MATS_OVER] = (bits >> 4) & 1; v[F_NOCLASSIFY_FROM] = (bits & 32) ? 1 : 1 << 30; v[F_MOTION] = (bits >> 6) & 1; v[F_TAIL_FROM] = t ? 3 : 12;
        check_case(v, en.s, en.e);
      }
      // the camera form's and the root cull's gates
      defaults();
      for (int bits = 0; bits < 16; bits++) for (int knob = -1; knob <= 1; knob++) for (int d : depths) {
        v[F_MOTION] = bits & 1; v[F_LENS] = (bits >> 1) & 1; v[F_CAM_COMPACT_OK] = (bits >> 2) & 1; v[F_MISS_SHARE_HIGH] = (bits >> 3) & 1;
        v[F_ROOT_CULL_KNOB] = knob; v[F_MAX_DEPTH] = d;
        check_case(v, en.s, en.e);
      }
    }
  }
  printf("scenes=%llu noengine=%llu engines=%zu cases=%llu planned=%llu refused=%llu refused_beyond_aggregate=%llu keys=%zu\n", n_scenes, n_noengine,
         engines.size(), n_cases, n_planned, n_refused, n_refused_beyond_aggregate, sizeof kKeys / sizeof kKeys[0]);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc == 2 && !strcmp(argv[1], "table")) return table();
  fprintf(stderr, "usage: plan_sweep sweep | table < rows\n");
  return 2;
}
