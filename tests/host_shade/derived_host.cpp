// CPU driver for the two material views of kernels/shade.hip.h (tests only): the shading device functions compiled as host
// C++ behind profiles/host_shade/hip/hip_runtime.h, like seam_host.cpp, but instantiated over BOTH views — MatRaw (every
// per-material constant computed at the call) and MatDerived (read from a DevMaterial that derive_material() filled once)
// — and in both forms the kernels run: the general one (prefixes raw_, drv_) and the SIMPLE one of simple-material tables
// (sraw_, sdrv_). Same signatures as the oracle drivers (oracle/ora_shade.c), so tests/test_shading_derived_host.py
// compares all of them record by record. Build: that test (g++ -O1 -ffp-contract=off -shared).
#include <cstddef>
#include <cstring>
#include <vector>
#include "shade.hip.h"

using namespace crt;
using namespace crt::dev;

static uint32_t g_tab[kSobolLdsWords];
static bool g_tab_ready = false;
static const uint32_t *sobol_tab() {
  if (!g_tab_ready) { sobol_tables_init(g_tab); g_tab_ready = true; }
  return g_tab;
}
static HitRec rec_of(const CrtShadeQuery &q) {
  HitRec r;
  r.p = v3(q.p[0], q.p[1], q.p[2]); r.normal = v3(q.normal[0], q.normal[1], q.normal[2]); r.t = q.t;
  r.front_face = q.front_face != 0;
  return r;
}
static void put(float d[3], V3 a) { d[0] = a.x; d[1] = a.y; d[2] = a.z; }

// The table as a view sees it: the raw records, or the records derived from them — once, before any query.
struct RawTable {
  const CrtMaterial *mats;
  RawTable(const CrtMaterial *m, size_t) : mats(m) {}
  MatRaw view(uint32_t i) const { return MatRaw{mats[i]}; }
};
struct DerivedTable {
  const CrtMaterial *mats;
  std::vector<DevMaterial> derived;
  DerivedTable(const CrtMaterial *m, size_t n) : mats(m), derived(n) {
    for (size_t i = 0; i < n; i++) derive_material(m[i], derived[i]);
  }
  MatDerived view(uint32_t i) const { return MatDerived{derived[i], mats[i]}; }
};

template <class Table, bool SIMPLE>
static void scatter_n(const CrtMaterial *mats, size_t n_mats, const CrtShadeQuery *qs, size_t n, CrtScatterSample *out) {
  const uint32_t *tab = sobol_tab();
  const Table table(mats, n_mats);
  for (size_t i = 0; i < n; i++) {
    std::memset(&out[i], 0, sizeof out[i]);
    if (qs[i].material >= n_mats) continue;
    Scatter sc;
    if (!mat_scatter<SIMPLE>(table.view(qs[i].material), v3(qs[i].ray_dir[0], qs[i].ray_dir[1], qs[i].ray_dir[2]), rec_of(qs[i]),
                             Sampler{qs[i].sampler_pattern, qs[i].sampler_index}, sc, tab)) continue;
    if (sc.medium) { DevMedium med; medium_from_material(mats[qs[i].material], med); sc.medium = med.present != 0; }  // as k_seam_scatter
    put(out[i].origin, sc.origin); put(out[i].dir, sc.dir); put(out[i].value, sc.value);
    out[i].some = 1; out[i].pdf = sc.pdf; out[i].flags = (sc.delta ? 1u : 0u) | (sc.medium ? 2u : 0u);
  }
}
template <class Table, bool SIMPLE>
static void eval_n(const CrtMaterial *mats, size_t n_mats, const CrtShadeQuery *qs, size_t n, CrtBsdfEval *out) {
  const Table table(mats, n_mats);
  for (size_t i = 0; i < n; i++) {
    std::memset(&out[i], 0, sizeof out[i]);
    if (qs[i].material >= n_mats) continue;
    V3 value; float pdf;
    if (!mat_eval<SIMPLE>(table.view(qs[i].material), v3(qs[i].ray_dir[0], qs[i].ray_dir[1], qs[i].ray_dir[2]), rec_of(qs[i]),
                          v3(qs[i].wi[0], qs[i].wi[1], qs[i].wi[2]), value, pdf)) continue;
    put(out[i].value, value); out[i].pdf = pdf; out[i].some = 1;
  }
}
template <class Table, bool SIMPLE>
static void emitted_n(const CrtMaterial *mats, size_t n_mats, const CrtShadeQuery *qs, size_t n, float *rgb) {
  const Table table(mats, n_mats);
  for (size_t i = 0; i < n; i++) {
    V3 e = splat(0.0f);
    if (qs[i].material < n_mats) e = mat_emitted_directional<SIMPLE>(table.view(qs[i].material), qs[i].cos_theta_o);
    put(rgb + 3 * i, e);
  }
}

extern "C" {

#define DRIVERS(prefix, Table, SIMPLE)                                                                                          \
  void prefix##_scatter_n(const CrtMaterial *m, size_t nm, const CrtShadeQuery *q, size_t n, CrtScatterSample *o) {            \
    scatter_n<Table, SIMPLE>(m, nm, q, n, o);                                                                                   \
  }                                                                                                                             \
  void prefix##_eval_n(const CrtMaterial *m, size_t nm, const CrtShadeQuery *q, size_t n, CrtBsdfEval *o) {                    \
    eval_n<Table, SIMPLE>(m, nm, q, n, o);                                                                                      \
  }                                                                                                                             \
  void prefix##_emitted_n(const CrtMaterial *m, size_t nm, const CrtShadeQuery *q, size_t n, float *o) {                       \
    emitted_n<Table, SIMPLE>(m, nm, q, n, o);                                                                                   \
  }
DRIVERS(raw, RawTable, false)
DRIVERS(drv, DerivedTable, false)
DRIVERS(sraw, RawTable, true)
DRIVERS(sdrv, DerivedTable, true)
#undef DRIVERS

// The derived records themselves (DevMaterial as dwords), for the test that pins their size and that they hold no NaN
// where a finite material goes in.
size_t derive_n(const CrtMaterial *mats, size_t n_mats, uint32_t *out_words) {
  for (size_t i = 0; i < n_mats; i++) {
    DevMaterial d;
    derive_material(mats[i], d);
    std::memcpy(out_words + i * (sizeof(DevMaterial) / 4), &d, sizeof d);
  }
  return sizeof(DevMaterial);
}

}  // extern "C"
