// The vertex function of unlit simple-material scenes (kernels/vertex_simple.hip.h: what k_shade_pipe's vertex step and
// k_camera_vertex both call) compiled as host C++ behind profiles/host_shade/hip/hip_runtime.h and run on random FIRST
// vertices — a camera path's constants: throughput 1, radiance 0, no vertex recorded, no previous vertex — under
// AddressSanitizer + UndefinedBehaviorSanitizer, through both material views (MatRaw, MatDerived).
// Each result is compared, bit for bit, with the same vertex put together from the seam's own call: mat_scatter on the
// raw record as kernels/shade_seam.hip drives it (k_seam_scatter: the general instance, the vertex domain's K_BSDF
// child), the emission of the record, and the integrator's update  beta = 1 * (1 * (value * cos / pdf)),
// L = 0 + (1 * 1) * emitted.  Exit 1 on the first difference.
//   bash profiles/host_shade/run_vertex.sh
#include <cstdio>
#include <cstdlib>
#include <random>
#include "vertex_simple.hip.h"
using namespace crt;
using namespace crt::dev;

static std::mt19937 rng(2468);
static float U() { return std::generate_canonical<float, 24>(rng); }
static float R(float a, float b) { return a + (b - a) * U(); }
static V3 rv(float a, float b) { return v3(R(a, b), R(a, b), R(a, b)); }

// a SIMPLE record: no coat, fuzz, thin film, transmission or subsurface anywhere
static CrtMaterial simple_material(int k) {
  CrtMaterial m;
  std::memset(&m, 0, sizeof m);
  float *f = reinterpret_cast<float *>(&m);
  for (size_t i = 0; i < sizeof(CrtMaterial) / 4; i++) f[i] = U();
  m.kind = (k % 11 == 0) ? CRT_MAT_EMISSIVE : CRT_MAT_OPENPBR;
  m.coat_weight = m.fuzz_weight = m.thin_film_weight = m.transmission_weight = m.subsurface_weight = 0.0f;
  m.transmission_depth = 0.0f;
  m.transmission_dispersion_scale = 0.0f;
  m.specular_ior = R(1.05f, 2.5f);
  m.coat_ior = R(1.1f, 2.0f);
  m.thin_film_ior = R(1.1f, 2.0f);
  m.thin_walled = 0u;
  if (k % 3) m.emission_luminance = 0.0f;  // most records do not emit
  if (k % 5 == 0) m.specular_weight = 0.0f;
  if (k % 7 == 0) m.base_metalness = 1.0f;
  return m;
}

static bool same(const V3 &a, const V3 &b) { return std::memcmp(&a, &b, sizeof(V3)) == 0; }

template <class MV>
static int check(const MV &mv, const CrtMaterial &m, const V3 &ro, const V3 &rd, const HitRec &rec, uint32_t pattern, uint32_t sample,
                 int depth, const uint32_t *tab, int it, const char *view, unsigned long long &n_alive, double &sum) {
  const VertexOut v = vertex_simple(mv, ro, rd, splat(1.0f), splat(0.0f), rec, pattern, sample, 0u, depth, false, tab);
  // the same vertex from the seam's call
  const Sampler vdom = new_domain(Sampler{pattern, sample}, 0);
  Scatter sc;
  sc.origin = sc.dir = sc.value = splat(0.0f); sc.pdf = 0.0f; sc.delta = false; sc.medium = false;
  const bool some = mat_scatter<false>(m, rd, rec, new_domain(vdom, K_BSDF), sc, tab);
  const V3 emitted = mat_emitted_directional<false>(m, fabs_(dot(normalize(rd), rec.normal)));
  const V3 one = splat(1.0f);
  V3 beta = one, L = splat(0.0f) + (one * one) * emitted;
  if (some) {
    const float cosine = sc.delta ? 1.0f : fabs_(dot(rec.normal, normalize(sc.dir)));
    beta = one * (one * ((sc.value * cosine) / sc.pdf));
  }
  bool ok = v.alive == some && same(v.beta, beta) && same(v.L, L) && v.closest == 1 && v.vertices == 1 && v.rr_tested == 0 &&
            v.rr_killed == 0 && v.escaped == 0 && v.depth_ended == 0;
  if (some) ok = ok && same(v.origin, sc.origin) && same(v.dir, sc.dir) && v.delta == sc.delta;
  if (!ok) {
    std::fprintf(stderr, "vertex %d (%s view) differs from the seam's: alive %d / %d, beta %.9g %.9g %.9g / %.9g %.9g %.9g\n", it, view,
                 (int)v.alive, (int)some, v.beta.x, v.beta.y, v.beta.z, beta.x, beta.y, beta.z);
    return 1;
  }
  n_alive += v.alive;
  sum += v.beta.x + v.beta.y + v.beta.z + v.L.x + v.L.y + v.L.z + v.origin.x + v.dir.x;
  return 0;
}

int main() {
  static uint32_t tab[kSobolLdsWords];
  sobol_tables_init(tab);
  unsigned long long n = 0, n_alive = 0, n_emit = 0, n_depth = 0;
  double sum = 0.0;
  for (int it = 0; it < 100000; it++) {
    const CrtMaterial m = simple_material(it);
    DevMaterial d;
    derive_material(m, d);
    const V3 ro = rv(-5.0f, 5.0f);
    V3 rd = rv(-1.0f, 1.0f);
    HitRec rec;
    rec.normal = normalize(rv(-1.0f, 1.0f));
    if (dot(rd, rec.normal) > 0.0f) rd = rd * -1.0f;  // the hit record's normal faces the ray
    rec.t = R(0.01f, 20.0f);
    rec.p = ro + rd * rec.t;
    rec.front_face = (it & 1) != 0;
    const uint32_t pattern = new_domain(new_domain(sampler_new(it & 255, (it >> 8) & 255, 0, it), 0), 1).pattern, sample = (uint32_t)(it % 512);
    const int depth = 1 + it % 32;
    if (check(MatRaw{m}, m, ro, rd, rec, pattern, sample, depth, tab, it, "raw", n_alive, sum)) return 1;
    if (check(MatDerived{d, m}, m, ro, rd, rec, pattern, sample, depth, tab, it, "derived", n_alive, sum)) return 1;
    const V3 e = mat_emitted_directional<true>(MatRaw{m}, 1.0f);
    n_emit += len2(e) > 0.0f;
    // the depth limit with no previous vertex: nothing is added, nothing goes on, one path ended at the limit
    const VertexOut z = vertex_simple(MatRaw{m}, ro, rd, splat(1.0f), splat(0.0f), rec, pattern, sample, 0u, 0, false, tab);
    if (z.alive || z.closest || z.vertices || z.depth_ended != 1 || !same(z.L, splat(0.0f)) || !same(z.beta, splat(1.0f))) {
      std::fprintf(stderr, "vertex %d at depth 0: not the depth-limit arm\n", it);
      return 1;
    }
    n_depth++;
    n++;
  }
  std::printf("vertices %llu alive %llu emitting %llu depth-limit %llu checksum %.17g\n", 2 * n, n_alive, n_emit, n_depth, sum);
  return 0;
}
