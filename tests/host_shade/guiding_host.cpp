// CPU twin of the guiding field's device functions (tests only): kernels/guiding.hip.h — the SAME source the seam kernels
// of kernels/guiding_seam.hip include, and for the guided bounce kernels/shade.hip.h — compiled as host C++ behind the HIP
// stand-in header profiles/host_shade/hip/hip_runtime.h and exported over arrays, so tests/test_guiding.py can compare
// it with the numpy restatement (tests/guiding_ref.py) bit for bit, and so that restatement takes its sincos / atan2
// from the device source. `image` is the byte image crt_guiding_image hands out (host memory).
// Build: tests/guiding_ref.py (g++ -O1 -ffp-contract=off -shared, as tests/volume_ref.py builds volume_host.cpp).
#include <cstddef>
#include <cstdint>
#include <cstring>

#define CRT_GUIDING_BOUNCE
#include "guiding.hip.h"
#include "../../include/crt_guiding.h"

using namespace crt;
using namespace crt::dev;

namespace {
GuideView view(const void *image) {
  const unsigned char *im = static_cast<const unsigned char *>(image);
  GuideHeader h;
  std::memcpy(&h, im, sizeof(h));
  GuideView V;
  V.snodes = reinterpret_cast<const GuideSNode *>(im + h.off_snodes);
  V.dnodes = reinterpret_cast<const GuideDNode *>(im + h.off_dnodes);
  V.n_snodes = h.n_snodes; V.n_dnodes = h.n_dnodes; V.s_depth = h.s_depth; V.d_depth = h.d_depth;
  for (int a = 0; a < 3; a++) { V.bmin[a] = h.bmin[a]; V.bmax[a] = h.bmax[a]; }
  V.alpha = h.alpha;
  return V;
}
uint32_t g_tab[kSobolLdsWords];
bool g_tab_ready = false;
const uint32_t *sobol_tab() {
  if (!g_tab_ready) { sobol_tables_init(g_tab); g_tab_ready = true; }
  return g_tab;
}
void put(float d[3], V3 a) { d[0] = a.x; d[1] = a.y; d[2] = a.z; }
}  // namespace

extern "C" {

void host_guide_sincos_n(const float *x, size_t n, float *s, float *c) { for (size_t i = 0; i < n; i++) sincos_det(x[i], s[i], c[i]); }
void host_guide_atan2_n(const float *y, const float *x, size_t n, float *o) { for (size_t i = 0; i < n; i++) o[i] = atan2_det(y[i], x[i]); }
void host_guide_dir_to_canonical_n(const float *d, size_t n, float *p) {
  for (size_t i = 0; i < n; i++) guide_dir_to_canonical(v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), p + 2 * i);
}
void host_guide_canonical_to_dir_n(const float *p, size_t n, float *d) { for (size_t i = 0; i < n; i++) put(d + 3 * i, guide_canonical_to_dir(p + 2 * i)); }
void host_guide_pcg_n(uint64_t state, size_t n, float *o) { for (size_t i = 0; i < n; i++) o[i] = guide_pcg_f32(state); }
void host_guide_luminance_n(const float *c, size_t n, float *o) { for (size_t i = 0; i < n; i++) o[i] = guide_luminance(v3(c[3 * i], c[3 * i + 1], c[3 * i + 2])); }

// DTree::sample / DTree::pdf in the canonical square (upstream's unit tests work there), on the tree governing pos[3]
void host_guide_dtree_sample_n(const void *image, const float *pos, const float *seeds, size_t n, float *p, float *pdf, uint32_t *some) {
  const GuideView V = view(image);
  const uint32_t root = guide_dtree_at(V, v3(pos[0], pos[1], pos[2]));
  for (size_t i = 0; i < n; i++) {
    p[2 * i] = p[2 * i + 1] = pdf[i] = 0.0f;
    some[i] = guide_dtree_sample(V, root, seeds[2 * i], seeds[2 * i + 1], p + 2 * i, pdf[i]) ? 1u : 0u;
  }
}
void host_guide_dtree_pdf_n(const void *image, const float *pos, const float *p, size_t n, float *pdf) {
  const GuideView V = view(image);
  const uint32_t root = guide_dtree_at(V, v3(pos[0], pos[1], pos[2]));
  for (size_t i = 0; i < n; i++) {
    float c[2] = {p[2 * i], p[2 * i + 1]};
    pdf[i] = guide_dtree_pdf(V, root, c);
  }
}

// the records k_guide_query writes, field by field
void host_guide_sample_n(const void *image, const CrtGuidingQuery *q, size_t n, CrtGuidingResult *out) {
  const GuideView V = view(image);
  for (size_t i = 0; i < n; i++) {
    std::memset(&out[i], 0, sizeof out[i]);
    V3 dir; float pdf; bool trained;
    const bool some = guide_field_sample(V, v3(q[i].pos[0], q[i].pos[1], q[i].pos[2]), q[i].seed_u, q[i].seed_v, dir, pdf, trained);
    put(out[i].dir, dir); out[i].pdf = pdf; out[i].some = some ? 1u : 0u; out[i].trained = trained ? 1u : 0u;
  }
}
void host_guide_pdf_n(const void *image, const CrtGuidingQuery *q, size_t n, CrtGuidingResult *out) {
  const GuideView V = view(image);
  for (size_t i = 0; i < n; i++) {
    std::memset(&out[i], 0, sizeof out[i]);
    bool trained;
    out[i].pdf = guide_field_pdf(V, v3(q[i].pos[0], q[i].pos[1], q[i].pos[2]), v3(q[i].dir[0], q[i].dir[1], q[i].dir[2]), trained);
    out[i].some = 1u; out[i].trained = trained ? 1u : 0u;
  }
}
// the record k_guide_scatter writes
void host_guide_scatter_n(const void *image, const CrtMaterial *mats, size_t n_mats, const CrtShadeQuery *qs, size_t n, CrtScatterSample *out) {
  const GuideView V = view(image);
  const uint32_t *tab = sobol_tab();
  for (size_t i = 0; i < n; i++) {
    std::memset(&out[i], 0, sizeof out[i]);
    if (qs[i].material >= n_mats) continue;
    HitRec rec;
    rec.p = v3(qs[i].p[0], qs[i].p[1], qs[i].p[2]); rec.normal = v3(qs[i].normal[0], qs[i].normal[1], qs[i].normal[2]);
    rec.t = qs[i].t; rec.front_face = qs[i].front_face != 0;
    Scatter sc;
    sc.origin = sc.dir = sc.value = splat(0.0f); sc.pdf = 0.0f; sc.delta = false; sc.medium = false;
    uint32_t flags = 0;
    const bool some = guide_sample_bounce(V, mats[qs[i].material], v3(qs[i].ray_dir[0], qs[i].ray_dir[1], qs[i].ray_dir[2]), rec,
                                          Sampler{qs[i].sampler_pattern, qs[i].sampler_index}, sc, flags, tab);
    if (!some) { out[i].flags = flags; continue; }
    put(out[i].origin, sc.origin); put(out[i].dir, sc.dir); put(out[i].value, sc.value);
    out[i].some = 1; out[i].pdf = sc.pdf; out[i].flags = (sc.delta ? 1u : 0u) | (sc.medium ? 2u : 0u) | flags;
  }
}
// Material::scatter_importance on the derived K_BSDF domain (the unguided estimator of the mixture test)
void host_guide_plain_scatter_n(const CrtMaterial *mats, size_t n_mats, const CrtShadeQuery *qs, size_t n, CrtScatterSample *out) {
  const uint32_t *tab = sobol_tab();
  for (size_t i = 0; i < n; i++) {
    std::memset(&out[i], 0, sizeof out[i]);
    if (qs[i].material >= n_mats) continue;
    HitRec rec;
    rec.p = v3(qs[i].p[0], qs[i].p[1], qs[i].p[2]); rec.normal = v3(qs[i].normal[0], qs[i].normal[1], qs[i].normal[2]);
    rec.t = qs[i].t; rec.front_face = qs[i].front_face != 0;
    Scatter sc;
    if (!guide_plain_scatter(mats[qs[i].material], v3(qs[i].ray_dir[0], qs[i].ray_dir[1], qs[i].ray_dir[2]), rec,
                             new_domain(Sampler{qs[i].sampler_pattern, qs[i].sampler_index}, kDomainBsdf), sc, tab)) continue;
    put(out[i].origin, sc.origin); put(out[i].dir, sc.dir); put(out[i].value, sc.value);
    out[i].some = 1; out[i].pdf = sc.pdf; out[i].flags = (sc.delta ? 1u : 0u) | (sc.medium ? 2u : 0u);
  }
}

}  // extern "C"
