// The camera-vertex rule (crust-render_amd/csrc/launch_plan.h: plan_launches, LaunchPlan::camera_vertex) on the CPU, driven
// by tests/test_camera_vertex_plan.py. Plain C++17 against the header alone.
//   camera_vertex_sweep    sweeps the inputs that decide the form, prints the case counts, exit 1 on the first violation
#include "sweep_common.h"

int main() {
  unsigned long long n_cases = 0, n_planned = 0, n_on = 0, n_trace_only = 0, n_on_full = 0, n_on_slim = 0, n_on_nocull = 0, n_on_modes = 0;
  const int nodes[] = {100, 5000};
  const int depths[] = {0, 1, 32};
  const uint32_t colds[] = {0, kColdAll};
  const int traces[] = {-1, 0, 2, 3};
  for (int direct = 0; direct < 2; direct++) for (int packets = 0; packets <= 5; packets += 5) for (int nd : nodes)
  for (int root = 0; root < 2; root++) for (int want = -1; want <= 1; want += 2) for (uint32_t cold : colds) {
    DevScene s{};
    s.direct_leaves = (uint32_t)direct; s.n_packets = (uint32_t)packets; s.has_packets = packets != 0;
    s.pool_stack = 6u; s.n_nodes = (uint32_t)nd; s.cold = cold; s.root = root ? 0u : CRT_INVALID_ID;
    EngineSelect e;
    if (select_engine(s, want, e, true) != CRT_OK) continue;
    for (int mats = 0; mats < 2; mats++) for (int lights = 0; lights < 2; lights++) for (int stats = 0; stats < 2; stats++)
    for (int ff = -1; ff <= 1; ff++) for (int d : depths) for (int compact = 0; compact < 2; compact++) for (int cull = 0; cull <= 1; cull++)
    for (int vol = 0; vol < 2; vol++) for (int partial = 0; partial < 2; partial++) for (int pipe = 0; pipe < 2; pipe++)
    for (int many = 0; many < 2; many++) for (int nocls = 0; nocls < 3; nocls++) for (int emit = 0; emit < 2; emit++)
    for (int slim = 0; slim < 2; slim++) for (int trace : traces) {
      const int swide = (d + pipe + many + nocls + emit) & 1;  // CRT_SHADE_WIDE=0 on every other case
      PlanInputs q;
      q.engine = e; q.scene = s;
      q.mats_kind = mats; q.n_lights = lights ? 2u : 0u; q.strategy = CRT_STRATEGY_POWER;
      q.n_materials = many ? 64 : 8; q.pipe_mat_max = 40; q.max_depth = (uint32_t)d;
      q.force_fused = ff; q.prefer_stage = true; q.stage_min_paths = 1000; q.total = 2000; q.stats = stats != 0;
      q.cam_compact_ok = compact != 0; q.root_cull_knob = cull; q.root_miss_share = 0.25f; q.volumes = vol != 0; q.partial_active = partial != 0;
      q.no_emitter = emit == 0; q.slim_state = slim; q.shade_pipe = pipe; q.shade_wide = swide ? -1 : 0;
      q.noclassify_from = nocls == 0 ? 0 : (nocls == 1 ? 1 : 1 << 30);
      q.camera_trace_knob = trace;
      snprintf(g_case, sizeof g_case, "direct %d packets %d nodes %d root %d want %d cold %u | mats %d lights %d stats %d fused %d depth %d "
               "compact %d cull %d volumes %d partial %d pipe %d many %d noclassify %d emit %d slim %d trace %d shade_wide %d", direct, packets,
               nd, root, want, cold, mats, lights, stats, ff, d, compact, cull, vol, partial, pipe, many, nocls, emit, slim, trace, swide);
      LaunchPlan pl[3];  // knob 0, 1, unset
      int rc[3];
      for (int k = 0; k < 3; k++) {
        q.camera_vertex_knob = k < 2 ? k : -1;
        rc[k] = plan_launches(q, pl[k]);
      }
      n_cases++;
      for (int k = 1; k < 3; k++) REQUIRE(rc[k] == rc[0] && same_before_camera_vertex(pl[0], pl[k]));  // the knob changes nothing the plan held before
      REQUIRE(!pl[0].camera_vertex);  // 0: the parent's launches
      if (rc[0] != CRT_OK) {
        for (int k = 0; k < 3; k++) REQUIRE(!pl[k].camera_vertex);
        continue;
      }
      n_planned++;
      const LaunchPlan &on = pl[1];
      // the rule, stated apart from the function: k_camera's form, the pipelined early shade, at least one bounce
      const bool want_on = on.camera_trace && !on.shade_early.none() && d >= 1;
      REQUIRE(on.camera_vertex == want_on && pl[2].camera_vertex == want_on);  // unset = 1
      if (want_on) {
        // what the two forms imply: per stage, unlit, simple materials whose table fits, the compact camera form, a first
        // bounce the pipelined kernel runs
        REQUIRE(!on.fused && !lights && mats == 0 && !many && pipe && on.cam_compact != 0 && on.noclassify_from > 0 && !stats && !vol && !partial);
        REQUIRE(on.shade_early.family == KF_SHADE_PIPE && !on.extend_deferred_key().none());
        REQUIRE(on.camera_mode == (trace == 2 ? 1u : (trace == 3 ? (1u << 8) : 0u)));  // the test forms still apply
        n_on++;
        n_on_slim += on.slim_state;
        n_on_full += !on.slim_state;
        n_on_nocull += !on.root_cull;
        n_on_modes += on.camera_mode != 0;
      } else if (on.camera_trace) {
        n_trace_only++;
      }
    }
  }
  printf("cases=%llu planned=%llu on=%llu trace_only=%llu on_slim=%llu on_full=%llu on_nocull=%llu on_modes=%llu\n", n_cases, n_planned, n_on,
         n_trace_only, n_on_slim, n_on_full, n_on_nocull, n_on_modes);
  return 0;
}
