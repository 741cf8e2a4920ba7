// plan_launches with PlanInputs::faces (crust-render_amd/csrc/crt_internal.h) over the input grid of plan_sweep.cpp,
// driven by tests/test_face_plan.py. Every case is planned with faces off, with faces on, and with faces on beside volumes:
// the rules of a textured render are required of the second plan, the absence of every textured form of the first, a
// refusal of the third. That a plan with faces off is the plan the parent made is pinned by tests/test_launch_plan.py
// against tests/golden/launch_plan_cases.npz, which this file leaves alone.
//   faces_sweep           prints the case counts, exit 1 on the first violation
#define main plan_sweep_main  // the sweep's fields, scene_of, inputs_of and REQUIRE; its own main is not this program's
#include "plan_sweep.cpp"
#undef main

#define CRT_KEY_ONLY(family, kernel, ...) CRT_INSTANCE_KEY(family, kernel, __VA_ARGS__),
static const InstanceKey kExtendFacesKeys[] = {CRT_INSTANCES_EXTEND_FACES(CRT_KEY_ONLY)};
static const InstanceKey kShadeFacesKeys[] = {CRT_INSTANCES_SHADE_FACES(CRT_KEY_ONLY)};
#undef CRT_KEY_ONLY
template <size_t N>
static bool is_key(const InstanceKey (&keys)[N], const InstanceKey &k) {
  for (const InstanceKey &o : keys)
    if (o == k) return true;
  return false;
}

static unsigned long long f_cases = 0, f_planned = 0, f_refused = 0, f_stats_refused = 0, f_volumes_refused = 0;

static void check_faces_case(const int *v, const DevScene &s, const EngineSelect &e) {
  g_case = v;
  f_cases++;
  PlanInputs q = inputs_of(v, s, e);
  REQUIRE(!q.faces);  // the default
  LaunchPlan p0;
  const int rc0 = plan_launches(q, p0);
  // faces off: no textured form anywhere
  REQUIRE(!p0.faces && p0.extend.family != KF_EXTEND_FACES && p0.shade.family != KF_SHADE_FACES);
  q.faces = true;
  {  // beside volumes: refused, whatever else holds
    PlanInputs both = q;
    both.volumes = true;
    LaunchPlan pb;
    REQUIRE(plan_launches(both, pb) == CRT_ERR_UNSUPPORTED && pb.extend.none() && pb.shade.none() && !pb.faces);
    f_volumes_refused++;
  }
  LaunchPlan pl;
  const int rc = plan_launches(q, pl);
  if (rc != CRT_OK) {
    f_refused++;
    REQUIRE(rc == CRT_ERR_UNSUPPORTED);
    REQUIRE(pl.path.none() && pl.extend.none() && pl.shade.none() && pl.shade_early.none() && pl.shadow_key.none() && !pl.faces);
    if (q.stats) f_stats_refused++;
    else REQUIRE(rc0 != CRT_OK);  // without the stats build, textures refuse nothing the image did not refuse already
    return;
  }
  f_planned++;
  REQUIRE(!q.stats);  // the stats build holds no textured instances
  const bool lit = q.n_lights > 0;
  // always per stage, whatever the batch size and CRT_FUSED: no fused kernel, no fused tail
  REQUIRE(pl.faces && !pl.fused && pl.tail_at == 0xffffffffu && pl.path.none());
  // no camera-trace, camera-vertex or pixel-table launch: the batch starts with generate, on full camera paths
  REQUIRE(!pl.camera_trace && !pl.camera_vertex && !pl.pixel_table && !pl.cull_root_lds && pl.camera_key().none() && pl.extend_deferred_key().none());
  REQUIRE(pl.cam_compact == 0);
  // no pipelined or slim shade; no volume form
  REQUIRE(pl.shade_early.none() && !pl.slim_state && pl.shade_slim_key().none() && !pl.volumes && pl.volume_key.none() && pl.shadow_volume_key.none());
  // the FACES shade key: the material class, the lights at infinity, the light list — raw records (no derived-table argument)
  REQUIRE(pl.shade.family == KF_SHADE_FACES && is_key(kShadeFacesKeys, pl.shade));
  REQUIRE(pl.shade.arg[0] == q.mats_kind && pl.shade.arg[1] == (q.has_env ? 2 : (q.has_inf_lights ? 1 : 0)) && pl.shade.arg[2] == (lit ? 1 : 0));
  // the FACES extend key: the width the per-stage plan picks for the image, the cold state that carries u, v
  REQUIRE(pl.extend.family == KF_EXTEND_FACES && is_key(kExtendFacesKeys, pl.extend));
  REQUIRE((pl.extend.arg[1] & (int)kColdUV) != 0 && pl.ext_cold == pl.extend.arg[1]);
  if (rc0 == CRT_OK && !p0.fused) REQUIRE(pl.extend.arg[0] == p0.extend.arg[1] && pl.shadow_key == p0.shadow_key && pl.wide == p0.wide);
  REQUIRE(engine_accepts(engine_of_width(e, s, pl.extend.arg[0]), s, pl.extend.arg[1]));
  REQUIRE(pl.shadow == (lit && q.strategy != CRT_STRATEGY_BSDF) && pl.shadow == !pl.shadow_key.none());
}

// plan_sweep.cpp's grid, restated (its sweep() calls its own check and takes no callback): the engine outcomes, then CORE
// crossed with each group of gates. The two grids must stay in step: tests/test_face_plan.py runs `plan_sweep sweep`
// beside this program and requires the same engine and case counts, so a grid changed in one file only fails there.
int main() {
  const int colds[] = {0, 1, 2, 3, 4, 7, 2 | 16, 7 | 16, 7 | 16 | 32};
  const int nodes[] = {100, 1500, 5000};
  struct Seen { DevScene s; EngineSelect e; };
  std::vector<Seen> engines;
  for (int direct = 0; direct < 2; direct++) for (int packets = 0; packets <= 5; packets += 5) for (int stack = 6; stack <= 10; stack += 4)
  for (int nd : nodes) for (int cold : colds) for (int root = 0; root < 2; root++) for (int want = -1; want <= 2; want++) {
    int v[kRowFields] = {};
    v[F_DIRECT] = direct; v[F_PACKETS] = packets; v[F_POOL_STACK] = stack; v[F_NODES] = nd; v[F_COLD] = cold; v[F_ROOT_VALID] = root;
    const DevScene s = scene_of(v);
    EngineSelect e;
    if (select_engine(s, want, e, true) != CRT_OK) continue;
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
    for (int mats = 0; mats < 3; mats++) for (int lights = 0; lights < 4; lights++) for (int drv = 0; drv < 2; drv++)
    for (int stats = 0; stats < 2; stats++) for (int ff = -1; ff <= 1; ff++) for (int big = 0; big < 2; big++) {
      auto defaults = [&] {
        v[F_MATS] = mats; v[F_LIGHTS] = lights; v[F_DERIVED] = drv; v[F_STATS] = stats; v[F_FORCE_FUSED] = ff; v[F_BIG_BATCH] = big;
        v[F_STRATEGY] = CRT_STRATEGY_POWER; v[F_TAIL_FROM] = 12; v[F_MAX_DEPTH] = 32; v[F_NOCLASSIFY_FROM] = 1 << 30; v[F_SHADE_WIDE] = -1;
        v[F_SHADE_PIPE] = 1; v[F_MAT_INDEX] = 0; v[F_PARTITION] = 0; v[F_MOTION] = 0; v[F_LENS] = 0; v[F_CAM_COMPACT_OK] = 1;
        v[F_ROOT_CULL_KNOB] = -1; v[F_MISS_SHARE_HIGH] = 1; v[F_MATS_OVER] = 0;
      };
      defaults();
      for (int strategy = CRT_STRATEGY_POWER; strategy <= CRT_STRATEGY_BSDF; strategy++) for (int t : tails) for (int d : depths) for (int n : ncfs) {
        v[F_STRATEGY] = strategy; v[F_TAIL_FROM] = t; v[F_MAX_DEPTH] = d; v[F_NOCLASSIFY_FROM] = n;
        check_faces_case(v, en.s, en.e);
      }
      defaults();
      for (int bits = 0; bits < 128; bits++) for (int t = 0; t < 2; t++) {
        v[F_SHADE_WIDE] = (bits & 1) ? 0 : -1; v[F_SHADE_PIPE] = (bits >> 1) & 1; v[F_MAT_INDEX] = (bits >> 2) & 1; v[F_PARTITION] = (bits >> 3) & 1;
        v[F_MATS_OVER] = (bits >> 4) & 1; v[F_NOCLASSIFY_FROM] = (bits & 32) ? 1 : 1 << 30; v[F_MOTION] = (bits >> 6) & 1; v[F_TAIL_FROM] = t ? 3 : 12;
        check_faces_case(v, en.s, en.e);
      }
      defaults();
      for (int bits = 0; bits < 16; bits++) for (int knob = -1; knob <= 1; knob++) for (int d : depths) {
        v[F_MOTION] = bits & 1; v[F_LENS] = (bits >> 1) & 1; v[F_CAM_COMPACT_OK] = (bits >> 2) & 1; v[F_MISS_SHARE_HIGH] = (bits >> 3) & 1;
        v[F_ROOT_CULL_KNOB] = knob; v[F_MAX_DEPTH] = d;
        check_faces_case(v, en.s, en.e);
      }
    }
  }
  printf("engines=%zu cases=%llu planned=%llu refused=%llu stats_refused=%llu volumes_refused=%llu extend_keys=%zu shade_keys=%zu\n", engines.size(),
         f_cases, f_planned, f_refused, f_stats_refused, f_volumes_refused, sizeof kExtendFacesKeys / sizeof kExtendFacesKeys[0],
         sizeof kShadeFacesKeys / sizeof kShadeFacesKeys[0]);
  return 0;
}
