// plan_launches with PlanInputs::volumes (crust-render_amd/csrc/launch_plan.h) over the input grid of plan_sweep.cpp,
// driven by tests/test_volume_render.py. Every case is planned twice — volumes off and on — and the rules of a volume
// render are required of the second plan, the absence of every volume form of the first. That a plan with volumes off is
// the plan the parent made is pinned by tests/test_launch_plan.py against tests/golden/launch_plan_cases.npz, which this
// file leaves alone.
//   volume_sweep          prints the case counts, exit 1 on the first violation
#include "sweep_common.h"

static const InstanceKey kVolKeys[] = {
#define CRT_KEY_ONLY(family, kernel, ...) CRT_INSTANCE_KEY(family, kernel, __VA_ARGS__),
    CRT_INSTANCES_SHADE_VOL(CRT_KEY_ONLY)
#undef CRT_KEY_ONLY
};
static bool is_vol_key(const InstanceKey &k) {
  for (const InstanceKey &o : kVolKeys)
    if (o == k) return true;
  return false;
}

static unsigned long long v_cases = 0, v_planned = 0, v_refused = 0, v_stats_refused = 0;

static void check_volume_case(const int *v, const DevScene &s, const EngineSelect &e) {
  v_cases++;
  PlanInputs q = inputs_of(v, s, e);
  REQUIRE(!q.volumes);  // the default
  LaunchPlan p0;
  const int rc0 = plan_launches(q, p0);
  // volumes off: no volume form anywhere
  REQUIRE(!p0.volumes && p0.volume_key.none() && p0.shadow_volume_key.none() && p0.shade.family != KF_SHADE_VOL);
  q.volumes = true;
  LaunchPlan pl;
  const int rc = plan_launches(q, pl);
  if (rc != CRT_OK) {
    v_refused++;
    REQUIRE(rc == CRT_ERR_UNSUPPORTED);
    REQUIRE(pl.path.none() && pl.extend.none() && pl.shade.none() && pl.shade_early.none() && pl.shadow_key.none() && pl.volume_key.none() &&
            pl.shadow_volume_key.none());
    if (q.stats) v_stats_refused++;
    else REQUIRE(rc0 != CRT_OK);  // without the stats build, volumes refuse nothing the image did not refuse already
    return;
  }
  v_planned++;
  REQUIRE(!q.stats);  // the stats build holds no volume stage
  const bool lit = q.n_lights > 0;
  // always per stage, whatever the batch size and CRT_FUSED; no fused tail; full camera paths; no root cull
  REQUIRE(pl.volumes && !pl.fused && pl.tail_at == 0xffffffffu && pl.path.none());
  REQUIRE(pl.cam_compact == 0 && !pl.root_cull);
  // no pipelined shade, no slim state; the VOL shade key
  REQUIRE(pl.shade_early.none() && !pl.slim_state && pl.shade_slim_key().none());
  REQUIRE(pl.shade.family == KF_SHADE_VOL && is_vol_key(pl.shade));
  REQUIRE(pl.shade.arg[0] == q.mats_kind && pl.shade.arg[1] == (q.has_env ? 2 : (q.has_inf_lights ? 1 : 0)) && pl.shade.arg[2] == (lit ? 1 : 0));
  // the two new kernels
  REQUIRE(pl.volume_key.family == KF_VOLUME);
  REQUIRE(pl.shadow == (lit && q.strategy != CRT_STRATEGY_BSDF));
  REQUIRE(pl.shadow_volume_key.none() == !pl.shadow && (pl.shadow_volume_key.none() || pl.shadow_volume_key.family == KF_SHADOW_VOLUME));
  REQUIRE(pl.shadow == !pl.shadow_key.none());
  // the traversal kernels are the per-stage plan's own
  REQUIRE(!pl.extend.none() && pl.extend.arg[0] == 0);
  if (rc0 == CRT_OK && !p0.fused) REQUIRE(pl.extend == p0.extend && pl.shadow_key == p0.shadow_key && pl.wide == p0.wide);
  REQUIRE(engine_accepts(engine_of_width(e, s, pl.extend.arg[1]), s, pl.extend.arg[2]));
}

int main() {  // plan_sweep.cpp's grid (sweep_common.h, sweep_grid) under check_volume_case
  const GridCounts g = sweep_grid(check_volume_case);
  printf("engines=%zu cases=%llu planned=%llu refused=%llu stats_refused=%llu vol_keys=%zu\n", g.engines, v_cases, v_planned, v_refused,
         v_stats_refused, sizeof kVolKeys / sizeof kVolKeys[0]);
  return 0;
}
