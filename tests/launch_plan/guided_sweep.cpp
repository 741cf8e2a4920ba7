// plan_launches with PlanInputs::guided (crust-render_amd/csrc/launch_plan.h) over the input grid of plan_sweep.cpp,
// driven by tests/test_guided_plan.py. Every case is planned with guided off, with guided on, and with guided on beside
// volumes and beside textures: the rules of a guided render are required of the second plan, the absence of every guided
// form of the first, a refusal of the last two. That a plan with guided off is the plan the parent made this sweep cannot
// show (it has no plan of the parent's to compare with): tests/test_launch_plan.py pins it against
// tests/golden/launch_plan_cases.npz, made before the input existed, which this change leaves alone.
//   guided_sweep          prints the case counts, exit 1 on the first violation
#include "sweep_common.h"

#define CRT_KEY_ONLY(family, kernel, ...) CRT_INSTANCE_KEY(family, kernel, __VA_ARGS__),
static const InstanceKey kShadeGuidedKeys[] = {CRT_INSTANCES_SHADE_GUIDED(CRT_KEY_ONLY)};
static const InstanceKey kShadeVolKeys[] = {CRT_INSTANCES_SHADE_VOL(CRT_KEY_ONLY)};
#undef CRT_KEY_ONLY
template <size_t N>
static bool is_key(const InstanceKey (&keys)[N], const InstanceKey &k) {
  for (const InstanceKey &o : keys)
    if (o == k) return true;
  return false;
}
static unsigned long long g_cases = 0, g_planned = 0, g_refused = 0, g_stats_refused = 0, g_volumes_refused = 0, g_faces_refused = 0;

static void check_guided_case(const int *v, const DevScene &s, const EngineSelect &e) {
  g_cases++;
  PlanInputs q = inputs_of(v, s, e);
  REQUIRE(!q.guided);  // the default
  LaunchPlan p0;
  (void)plan_launches(q, p0);
  // guided off: no guided form anywhere
  REQUIRE(!p0.guided && p0.shade.family != KF_SHADE_GUIDED);
  // the per-stage plan of the same inputs without a tail (what a detached renderer runs under CRT_FUSED=0,
  // CRT_TAIL_FROM=0 — no k_path instance, which a guided batch never launches): extend and shadow come from it
  PlanInputs qs = q;
  qs.force_fused = 0;
  qs.tail_from = 0;
  LaunchPlan ps;
  const int rcs = plan_launches(qs, ps);
  REQUIRE(!ps.guided);
  q.guided = true;
  {  // beside volumes, beside textures: refused, whatever else holds
    PlanInputs both = q;
    both.volumes = true;
    LaunchPlan pb;
    REQUIRE(plan_launches(both, pb) == CRT_ERR_UNSUPPORTED && pb.extend.none() && pb.shade.none() && !pb.guided);
    g_volumes_refused++;
    both = q;
    both.faces = true;
    REQUIRE(plan_launches(both, pb) == CRT_ERR_UNSUPPORTED && pb.extend.none() && pb.shade.none() && !pb.guided && !pb.faces);
    g_faces_refused++;
  }
  LaunchPlan pl;
  const int rc = plan_launches(q, pl);
  if (rc != CRT_OK) {
    g_refused++;
    REQUIRE(rc == CRT_ERR_UNSUPPORTED);
    REQUIRE(pl.path.none() && pl.extend.none() && pl.shade.none() && pl.shade_early.none() && pl.shadow_key.none() && !pl.guided);
    if (q.stats) g_stats_refused++;
    else REQUIRE(rcs != CRT_OK);  // without the stats build, guiding refuses nothing the image's per-stage plan did not refuse already
    return;
  }
  g_planned++;
  REQUIRE(!q.stats);  // the stats build holds no guided instances
  const bool lit = q.n_lights > 0;
  // always per stage, whatever the batch size and CRT_FUSED: no fused kernel, no fused tail
  REQUIRE(pl.guided && !pl.fused && pl.tail_at == 0xffffffffu && pl.path.none());
  // no camera-trace, camera-vertex or pixel-table launch: the batch starts with generate, on full camera paths
  REQUIRE(!pl.camera_trace && !pl.camera_vertex && !pl.pixel_table && !pl.cull_root_lds && pl.camera_key().none() && pl.extend_deferred_key().none());
  REQUIRE(pl.cam_compact == 0);
  // no pipelined or slim shade; no volume and no textured form
  REQUIRE(pl.shade_early.none() && !pl.slim_state && pl.shade_slim_key().none() && !pl.volumes && pl.volume_key.none() &&
          pl.shadow_volume_key.none() && !pl.faces);
  // the GUIDED shade key: the material class, the lights at infinity, the light list — raw records; k_shade_vol's twelve rows
  REQUIRE(pl.shade.family == KF_SHADE_GUIDED && is_key(kShadeGuidedKeys, pl.shade));
  REQUIRE(pl.shade.arg[0] == q.mats_kind && pl.shade.arg[1] == (q.has_env ? 2 : (q.has_inf_lights ? 1 : 0)) && pl.shade.arg[2] == (lit ? 1 : 0));
  {
    InstanceKey as_vol = pl.shade;
    as_vol.family = KF_SHADE_VOL;
    REQUIRE(is_key(kShadeVolKeys, as_vol));
  }
  // extend and shadow: the unbound per-stage plan's instances, an ordinary k_extend
  REQUIRE(pl.extend.family == KF_EXTEND);
  REQUIRE(rcs == CRT_OK && pl.extend == ps.extend && pl.shadow_key == ps.shadow_key && pl.wide == ps.wide && pl.ext_cold == ps.ext_cold);
  REQUIRE(pl.shadow == (lit && q.strategy != CRT_STRATEGY_BSDF) && pl.shadow == !pl.shadow_key.none());
}

int main() {  // plan_sweep.cpp's grid (sweep_common.h, sweep_grid) under check_guided_case
  const GridCounts g = sweep_grid(check_guided_case);
  printf("engines=%zu cases=%llu planned=%llu refused=%llu stats_refused=%llu volumes_refused=%llu faces_refused=%llu shade_keys=%zu\n", g.engines,
         g_cases, g_planned, g_refused, g_stats_refused, g_volumes_refused, g_faces_refused, sizeof kShadeGuidedKeys / sizeof kShadeGuidedKeys[0]);
  return 0;
}
