// plan_launches with PlanInputs::faces (crust-render_amd/csrc/launch_plan.h) over the input grid of plan_sweep.cpp,
// driven by tests/test_face_plan.py. Every case is planned with faces off, with faces on, and with faces on beside volumes:
// the rules of a textured render are required of the second plan, the absence of every textured form of the first, a
// refusal of the third. That a plan with faces off is the plan the parent made is pinned by tests/test_launch_plan.py
// against tests/golden/launch_plan_cases.npz, which this file leaves alone.
//   faces_sweep           prints the case counts, exit 1 on the first violation
#include "sweep_common.h"

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

int main() {  // plan_sweep.cpp's grid (sweep_common.h, sweep_grid) under check_faces_case
  const GridCounts g = sweep_grid(check_faces_case);
  printf("engines=%zu cases=%llu planned=%llu refused=%llu stats_refused=%llu volumes_refused=%llu extend_keys=%zu shade_keys=%zu\n", g.engines,
         f_cases, f_planned, f_refused, f_stats_refused, f_volumes_refused, sizeof kExtendFacesKeys / sizeof kExtendFacesKeys[0],
         sizeof kShadeFacesKeys / sizeof kShadeFacesKeys[0]);
  return 0;
}
