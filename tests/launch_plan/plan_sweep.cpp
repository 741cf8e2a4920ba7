// The renderer's launch planning (crust-render_amd/csrc/launch_plan.h: select_engine, plan_launches) on the CPU, driven
// by tests/test_launch_plan.py. Plain C++17 against the header alone; built once per build-switch tuple (-DCRT_..._BUILD).
//   plan_sweep sweep          the property sweep over the input grid; prints the case counts, exit 1 on the first violation
//   plan_sweep table < rows   one decision line per input row (kRowFields integers): the parent's decision table
#include <string>

#include "sweep_common.h"

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

static int sweep() {  // the shared grid (sweep_common.h, sweep_grid) under check_case
  const GridCounts g = sweep_grid(check_case);
  printf("scenes=%llu noengine=%llu engines=%zu cases=%llu planned=%llu refused=%llu refused_beyond_aggregate=%llu keys=%zu\n", g.scenes, g.noengine,
         g.engines, n_cases, n_planned, n_refused, n_refused_beyond_aggregate, sizeof kKeys / sizeof kKeys[0]);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc == 2 && !strcmp(argv[1], "table")) return table();
  fprintf(stderr, "usage: plan_sweep sweep | table < rows\n");
  return 2;
}
