// The camera-trace rule (crust-render_amd/csrc/launch_plan.h: plan_launches, LaunchPlan::camera_trace) on the CPU, driven by
// tests/test_camera_trace_plan.py. Plain C++17 against the header alone.
//   camera_sweep    sweeps the inputs that decide the form, prints the case counts, exit 1 on the first violation
#include "sweep_common.h"

static const InstanceKey kDeferredKeys[] = {
#define CRT_KEY_ONLY(family, kernel, ...) CRT_INSTANCE_KEY(family, kernel, __VA_ARGS__),
    CRT_INSTANCES_EXTEND_DEFERRED(CRT_KEY_ONLY)};
static const InstanceKey kExtendKeys[] = {CRT_INSTANCES_EXTEND(CRT_KEY_ONLY)};

int main() {
  unsigned long long n_cases = 0, n_planned = 0, n_on = 0, n_on_default = 0, n_on_nocull = 0, n_large_forced = 0;
  const int nodes[] = {100, 1500, 5000};
  const int depths[] = {0, 1, 32};
  const uint32_t colds[] = {0, kColdAll};
  for (int direct = 0; direct < 2; direct++) for (int packets = 0; packets <= 5; packets += 5) for (int nd : nodes)
  for (int root = 0; root < 2; root++) for (int want = -1; want <= 2; want++) for (uint32_t cold : colds) for (int deep = 0; deep < 2; deep++) {
    DevScene s{};
    s.direct_leaves = (uint32_t)direct; s.n_packets = (uint32_t)packets; s.has_packets = packets != 0;
    s.pool_stack = deep ? 10u : 6u; s.n_nodes = (uint32_t)nd; s.cold = cold; s.root = root ? 0u : CRT_INVALID_ID;
    EngineSelect e;
    if (select_engine(s, want, e, true) != CRT_OK) continue;
    for (int mats = 0; mats < 3; mats++) for (int lights = 0; lights < 2; lights++) for (int stats = 0; stats < 2; stats++)
    for (int ff = -1; ff <= 1; ff++) for (int big = 0; big < 2; big++) for (int d : depths) for (int lens = 0; lens < 2; lens++)
    for (int motion = 0; motion < 2; motion++) for (int compact = 0; compact < 2; compact++) for (int cull = -1; cull <= 1; cull++)
    for (int vol = 0; vol < 2; vol++) for (int partial = 0; partial < 2; partial++) for (int inf = 0; inf < 2; inf++) {
      if (inf && !lights) continue;
      PlanInputs q;
      q.engine = e; q.scene = s;
      q.mats_kind = mats; q.n_lights = lights ? 2u : 0u; q.has_inf_lights = inf != 0; q.strategy = CRT_STRATEGY_POWER;
      q.n_materials = 8; q.pipe_mat_max = 40; q.max_depth = (uint32_t)d; q.lens = lens != 0; q.has_motion = motion != 0;
      q.force_fused = ff; q.prefer_stage = true; q.stage_min_paths = 1000; q.total = big ? 2000 : 500; q.stats = stats != 0;
      q.cam_compact_ok = compact != 0; q.root_cull_knob = cull; q.root_miss_share = 0.25f; q.volumes = vol != 0; q.partial_active = partial != 0;
      q.no_emitter = true;
      snprintf(g_case, sizeof g_case, "direct %d packets %d nodes %d root %d want %d cold %u deep %d | mats %d lights %d stats %d fused %d big %d "
               "depth %d lens %d motion %d compact %d cull %d volumes %d partial %d inf %d", direct, packets, nd, root, want, cold, deep, mats,
               lights, stats, ff, big, d, lens, motion, compact, cull, vol, partial, inf);
      LaunchPlan pl[5];  // knob 0, 1, 2, 3, unset
      int rc[5];
      for (int k = 0; k < 5; k++) {
        q.camera_trace_knob = k < 4 ? k : -1;
        rc[k] = plan_launches(q, pl[k]);
      }
      n_cases++;
      for (int k = 1; k < 5; k++) REQUIRE(rc[k] == rc[0] && same_before_camera_trace(pl[0], pl[k]));  // the knob changes nothing the plan held before
      REQUIRE(!pl[0].camera_trace && pl[0].camera_mode == 0 && pl[0].extend_deferred_key().none());  // 0: the parent's launches
      if (rc[0] != CRT_OK) {
        for (int k = 0; k < 5; k++) REQUIRE(!pl[k].camera_trace && pl[k].extend_deferred_key().none());
        continue;
      }
      n_planned++;
      const LaunchPlan &on = pl[1], &dflt = pl[4];
      // the rule, stated apart from the function: per-stage, the compact camera form, the flat four-wave engine instance
      // without cold state on an image with packets and a root, at least one bounce, every pixel sampling, not the stats
      // build, not a volume render
      const bool want_on = !on.fused && on.cam_compact != 0 && on.extend.family == KF_EXTEND && on.extend.arg[0] == 0 && on.extend.arg[1] == 1 &&
                           on.extend.arg[2] == 0 && s.n_packets > 0 && s.direct_leaves == 0 && s.root != CRT_INVALID_ID && d >= 1 && !partial &&
                           !stats && !vol;
      REQUIRE(on.camera_trace == want_on);
      REQUIRE(pl[2].camera_trace == want_on && pl[3].camera_trace == want_on);
      REQUIRE(dflt.camera_trace == (want_on && s.n_nodes <= kCameraTraceMaxNodes));  // unset: small trees only
      if (want_on) {
        // what the compact form implies: unlit, pinhole, static
        REQUIRE(!lights && !lens && !motion && compact && on.wide);
        REQUIRE(on.cam_compact == (on.root_cull ? 2u : 1u));
        REQUIRE(on.camera_mode == 0 && pl[2].camera_mode == 1u && pl[3].camera_mode == (1u << 8));
        const InstanceKey k = on.extend_deferred_key();
        REQUIRE(k.family == KF_EXTEND_DEFERRED && k.arg[0] == on.extend.arg[0] && k.arg[1] == on.extend.arg[1] && k.arg[2] == on.extend.arg[2]);
        bool held = false, extend_held = false;
        for (const InstanceKey &h : kDeferredKeys) held = held || h == k;
        for (const InstanceKey &h : kExtendKeys) extend_held = extend_held || h == on.extend;
        REQUIRE(held && extend_held);
        n_on++;
        n_on_default += dflt.camera_trace;
        n_on_nocull += !on.root_cull;
        n_large_forced += s.n_nodes > kCameraTraceMaxNodes;
      } else {
        for (int k = 1; k < 5; k++) REQUIRE(pl[k].camera_mode == 0 && pl[k].extend_deferred_key().none());
      }
    }
  }
  printf("cases=%llu planned=%llu on=%llu on_default=%llu on_nocull=%llu large_forced=%llu\n", n_cases, n_planned, n_on, n_on_default,
         n_on_nocull, n_large_forced);
  return 0;
}
