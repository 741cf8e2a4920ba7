// The slim path state's rule (crust-render_amd/csrc/launch_plan.h: plan_launches, LaunchPlan::slim_state,
// table_has_no_emitter) on the CPU, driven by tests/test_slim_state_plan.py. Plain C++17 against the header alone.
//   slim_sweep      sweeps the inputs that decide the form, prints the case counts, exit 1 on the first violation
#include <limits>

#include "sweep_common.h"

static const InstanceKey kSlimKeys[] = {
#define CRT_KEY_ONLY(family, kernel, ...) CRT_INSTANCE_KEY(family, kernel, __VA_ARGS__),
    CRT_INSTANCES_SHADE_PIPE_SLIM(CRT_KEY_ONLY)};
static const InstanceKey kPipeKeys[] = {CRT_INSTANCES_SHADE_PIPE(CRT_KEY_ONLY)};

static CrtMaterial record(uint32_t kind, float r, float g, float b, float lum) {
  CrtMaterial m;
  memset(&m, 0, sizeof m);
  m.kind = kind;
  m.emission_color[0] = r; m.emission_color[1] = g; m.emission_color[2] = b;
  m.emission_luminance = lum;
  return m;
}

static void emitter_cases() {
  snprintf(g_case, sizeof g_case, "table_has_no_emitter");
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  struct Case { CrtMaterial m; bool dark; };
  const Case cases[] = {
      {record(CRT_MAT_OPENPBR, 1, 1, 1, 0), true},          // the default record: a colour, luminance 0
      {record(CRT_MAT_OPENPBR, 1, 1, 1, -0.0f), true},
      {record(CRT_MAT_OPENPBR, 0, 0, 0, 5), true},          // a luminance, no colour
      {record(CRT_MAT_OPENPBR, 0, -0.0f, 0, 5), true},
      {record(CRT_MAT_OPENPBR, 1, 0.6f, 0.2f, 2), false},   // emits
      {record(CRT_MAT_OPENPBR, 0, 0, 1e-30f, 1e-30f), false},  // no arithmetic: an underflowing product still counts
      {record(CRT_MAT_OPENPBR, nan, 0, 0, 0), false},
      {record(CRT_MAT_OPENPBR, 0, 0, 0, nan), false},
      {record(CRT_MAT_OPENPBR, 1, 1, 1, nan), false},
      {record(CRT_MAT_OPENPBR, 0, 0, 0, inf), false},       // 0 * inf is a NaN
      {record(CRT_MAT_OPENPBR, inf, 1, 1, 0), false},
      {record(CRT_MAT_EMISSIVE, 0, 0, 0, 1), true},         // an Emissive's radiance is its colour as it stands
      {record(CRT_MAT_EMISSIVE, 0, 0, 0, inf), true},
      {record(CRT_MAT_EMISSIVE, 0, 0, 0, nan), false},      // a NaN anywhere
      {record(CRT_MAT_EMISSIVE, 1, 1, 1, 0), false},        // ... whatever the luminance
      {record(CRT_MAT_EMISSIVE, 0, 0, 4, 1), false},
      {record(CRT_MAT_EMISSIVE, nan, 0, 0, 1), false},
  };
  REQUIRE(table_has_no_emitter(nullptr, 0));
  const CrtMaterial dark = record(CRT_MAT_OPENPBR, 1, 1, 1, 0);
  for (const Case &c : cases) {
    REQUIRE(table_has_no_emitter(&c.m, 1) == c.dark);
    for (int at = 0; at < 3; at++) {  // one record decides for the table, wherever it sits
      CrtMaterial t[3] = {dark, dark, dark};
      t[at] = c.m;
      REQUIRE(table_has_no_emitter(t, 3) == c.dark);
    }
  }
}

int main() {
  emitter_cases();
  unsigned long long n_cases = 0, n_planned = 0, n_piped = 0, n_slim = 0, n_slim_stats = 0;
  const int nodes[] = {100, 1500, 5000};
  const int tails[] = {0, 2, 12}, ncfs[] = {0, 1, 3, 1 << 30}, depths[] = {0, 3, 32};
  for (int direct = 0; direct < 2; direct++) for (int packets = 0; packets <= 5; packets += 5) for (int nd : nodes)
  for (int root = 0; root < 2; root++) for (int want = -1; want <= 2; want++) {
    DevScene s{};
    s.direct_leaves = (uint32_t)direct; s.n_packets = (uint32_t)packets; s.has_packets = packets != 0;
    s.pool_stack = 6; s.n_nodes = (uint32_t)nd; s.cold = 0; s.root = root ? 0u : CRT_INVALID_ID;
    EngineSelect e;
    if (select_engine(s, want, e, true) != CRT_OK) continue;
    for (int mats = 0; mats < 3; mats++) for (int lights = 0; lights < 2; lights++) for (int pipe = 0; pipe < 2; pipe++)
    for (int stats = 0; stats < 2; stats++) for (int ff = -1; ff <= 1; ff++) for (int big = 0; big < 2; big++)
    for (int t : tails) for (int ncf : ncfs) for (int d : depths) for (int over = 0; over < 2; over++) for (int drv = 0; drv < 2; drv++)
    for (int dark = 0; dark < 2; dark++) {
      PlanInputs q;
      q.engine = e; q.scene = s;
      q.mats_kind = mats; q.mat_derived = drv != 0; q.n_lights = lights ? 2u : 0u; q.strategy = CRT_STRATEGY_POWER;
      q.n_materials = (uint32_t)(40 + over); q.pipe_mat_max = 40; q.max_depth = (uint32_t)d;
      q.force_fused = ff; q.prefer_stage = true; q.stage_min_paths = 1000; q.total = big ? 2000 : 500; q.stats = stats != 0;
      q.tail_from = t; q.noclassify_from = ncf; q.shade_pipe = pipe; q.root_miss_share = 0.25f;
      q.shade_pipe_build = true; q.root_cull_build = true;
      q.no_emitter = dark != 0;
      snprintf(g_case, sizeof g_case, "direct %d packets %d nodes %d root %d want %d | mats %d lights %d pipe %d stats %d fused %d big %d tail %d "
               "noclassify %d depth %d over %d drv %d no_emitter %d", direct, packets, nd, root, want, mats, lights, pipe, stats, ff, big, t, ncf, d,
               over, drv, dark);
      LaunchPlan off, on;
      q.slim_state = 0;
      const int rc_off = plan_launches(q, off);
      q.slim_state = 1;
      const int rc_on = plan_launches(q, on);
      n_cases++;
      REQUIRE(rc_off == rc_on && same_before_slim(off, on));  // the knob changes nothing the plan held before
      REQUIRE(!off.slim_state && off.shade_slim_key().none());
      if (rc_on != CRT_OK) { REQUIRE(!on.slim_state && on.shade_slim_key().none()); continue; }
      n_planned++;
      n_piped += on.shade_piped();
      // the rule: the pipelined instance runs, and nothing in the table emits
      REQUIRE(on.slim_state == (on.shade_piped() && dark != 0));
      if (on.slim_state) {  // ... so whatever keeps the pipelined instance away keeps the form away
        REQUIRE(!on.fused && on.wide && mats == 0 && lights == 0 && pipe != 0 && !over && ncf > 0 && shade_pipe_fits(q));
        const InstanceKey k = on.shade_slim_key();
        REQUIRE(k.family == KF_SHADE_PIPE && k.arg[0] == on.shade_early.arg[0] && k.arg[0] == (drv ? 1 : 0) && k.arg[1] == 1);
        bool held = false, early_held = false;
        for (const InstanceKey &h : kSlimKeys) held = held || h == k;
        for (const InstanceKey &h : kPipeKeys) early_held = early_held || h == on.shade_early;
        REQUIRE(held && early_held);
        n_slim++;
        n_slim_stats += stats;
      } else {
        REQUIRE(on.shade_slim_key().none());
      }
    }
  }
  printf("cases=%llu planned=%llu piped=%llu slim=%llu slim_stats=%llu\n", n_cases, n_planned, n_piped, n_slim, n_slim_stats);
  return 0;
}
