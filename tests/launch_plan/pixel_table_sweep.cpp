// The per-pixel camera table's rule (crust-render_amd/csrc/launch_plan.h: plan_launches, LaunchPlan::pixel_table) on the
// CPU, driven by tests/test_pixel_table_plan.py. Plain C++17 against the header alone.
//   pixel_table_sweep    sweeps the inputs that decide the form, prints the case counts, exit 1 on the first violation
#include "sweep_common.h"

int main() {
  unsigned long long n_cases = 0, n_planned = 0, n_on = 0, n_on_vertex = 0, n_on_trace = 0, n_on_modes = 0, n_unready = 0, n_lds = 0;
  const int nodes[] = {100, 5000};
  const int depths[] = {0, 1, 32};
  const int traces[] = {-1, 0, 1, 2, 3};
  for (int direct = 0; direct < 2; direct++) for (int packets = 0; packets <= 5; packets += 5) for (int nd : nodes)
  for (int root = 0; root < 2; root++) for (int want = -1; want <= 1; want += 2) {
    DevScene s{};
    s.direct_leaves = (uint32_t)direct; s.n_packets = (uint32_t)packets; s.has_packets = packets != 0;
    s.pool_stack = 6u; s.n_nodes = (uint32_t)nd; s.cold = 0; s.root = root ? 0u : CRT_INVALID_ID;
    EngineSelect e;
    if (select_engine(s, want, e, true) != CRT_OK) continue;
    for (int mats = 0; mats < 2; mats++) for (int lights = 0; lights < 2; lights++) for (int stats = 0; stats < 2; stats++)
    for (int ff = -1; ff <= 1; ff++) for (int d : depths) for (int compact = 0; compact < 2; compact++) for (int cull = 0; cull <= 1; cull++)
    for (int vol = 0; vol < 2; vol++) for (int partial = 0; partial < 2; partial++) for (int pipe = 0; pipe < 2; pipe++)
    for (int motion = 0; motion < 2; motion++) for (int lens = 0; lens < 2; lens++) for (int slim = 0; slim < 2; slim++)
    for (int vertex = -1; vertex <= 1; vertex++) for (int trace : traces) for (int ready = 0; ready < 2; ready++) {
      PlanInputs q;
      q.engine = e; q.scene = s;
      q.mats_kind = mats; q.n_lights = lights ? 2u : 0u; q.strategy = CRT_STRATEGY_POWER;
      q.n_materials = 8; q.pipe_mat_max = 40; q.max_depth = (uint32_t)d;
      q.force_fused = ff; q.prefer_stage = true; q.stage_min_paths = 1000; q.total = 2000; q.stats = stats != 0;
      q.cam_compact_ok = compact != 0; q.root_cull_knob = cull; q.root_miss_share = 0.25f; q.volumes = vol != 0; q.partial_active = partial != 0;
      q.no_emitter = true; q.slim_state = slim; q.shade_pipe = pipe; q.has_motion = motion != 0; q.lens = lens != 0;
      q.camera_trace_knob = trace; q.camera_vertex_knob = vertex; q.pixel_table_ready = ready != 0;
      snprintf(g_case, sizeof g_case, "direct %d packets %d nodes %d root %d want %d | mats %d lights %d stats %d fused %d depth %d compact %d "
               "cull %d volumes %d partial %d pipe %d motion %d lens %d slim %d vertex %d trace %d ready %d", direct, packets, nd, root, want,
               mats, lights, stats, ff, d, compact, cull, vol, partial, pipe, motion, lens, slim, vertex, trace, ready);
      LaunchPlan pl[3];  // knob 0, 1, unset
      int rc[3];
      // the other knob of the camera launch rides along: CRT_CULL_ROOT_LDS 0 / 1 / unset
      const int lds = (d + mats + vertex + trace + ready) % 3 - 1;
      q.cull_root_lds_knob = 0; q.pixel_table_knob = 0;
      LaunchPlan none;
      const int rc_none = plan_launches(q, none);
      REQUIRE(!none.pixel_table && !none.cull_root_lds);  // all 0: the parent's launches
      q.cull_root_lds_knob = lds;
      for (int k = 0; k < 3; k++) {
        q.pixel_table_knob = k < 2 ? k : -1;
        rc[k] = plan_launches(q, pl[k]);
      }
      n_cases++;
      REQUIRE(rc_none == rc[0] && same_before_pixel_table(none, pl[0]));
      for (int k = 1; k < 3; k++) REQUIRE(rc[k] == rc[0] && same_before_pixel_table(pl[0], pl[k]));  // the knobs change nothing the plan held before
      REQUIRE(!pl[0].pixel_table);  // 0: the computed form
      for (int k = 0; k < 3; k++) {
        // the root from LDS: a camera launch that culls, the root at node 0
        REQUIRE(pl[k].cull_root_lds == (rc[k] == CRT_OK && pl[k].camera_trace && pl[k].root_cull && lds != 0 && root != 0));
        n_lds += pl[k].cull_root_lds;
      }
      if (rc[0] != CRT_OK) {
        for (int k = 0; k < 3; k++) REQUIRE(!pl[k].pixel_table);
        continue;
      }
      n_planned++;
      const LaunchPlan &on = pl[1];
      // the rule, stated apart from the function: a camera launch runs, and the renderer holds a table
      const bool want_on = on.camera_trace && ready;
      REQUIRE(on.pixel_table == want_on && pl[2].pixel_table == want_on);  // unset = 1
      if (on.camera_trace && !ready) n_unready++;
      if (want_on) {
        // what a camera launch implies, and the table's form relies on: every owned pixel sampling, a static pinhole batch,
        // one launch per stage, not the stats build
        REQUIRE(!partial && !motion && !lens && !on.fused && !stats && !vol && !lights && on.cam_compact != 0);
        n_on++;
        n_on_vertex += on.camera_vertex;
        n_on_trace += !on.camera_vertex;
        n_on_modes += on.camera_mode != 0;
      }
    }
  }
  printf("cases=%llu planned=%llu on=%llu on_vertex=%llu on_trace=%llu on_modes=%llu unready=%llu root_lds=%llu\n", n_cases,
         n_planned, n_on, n_on_vertex, n_on_trace, n_on_modes, n_unready, n_lds);
  return 0;
}
