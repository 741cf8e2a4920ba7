// The vertex step of an unlit simple-material scene as a function: one iteration of trace_path's loop body for a path
// that hit a surface (tracer.rs:1118-1149, :1372-1381, :1459-1523) where the scene has no lights and no media and the
// material table holds simple records only. One source for its two callers — the pipelined shade kernel's VERTEX step
// (pathtrace.hip, shade_segment_pipe), which hands it a path's state out of its staging block, and k_camera_vertex, which
// hands it a camera path's constants right behind the ray's traversal — and for the host build of its check
// (profiles/host_shade/vertex_host.cpp, behind the stand-in <hip/hip_runtime.h>).
//
// The state comes in as values and the result goes out as values: the callers keep their own loads, queues and stores.
// A caller that passes literals (a camera path: record count 0, no previous vertex, throughput 1, radiance 0) has the
// roulette and the previous-vertex arms folded away; the arithmetic that remains is the same IEEE operations in the same
// order (-ffp-contract=off), so the two callers agree bit for bit.
#pragma once

#include "shade.hip.h"

namespace crt {
namespace dev {

enum { K_NEE = 0, K_NEE_SHADOW = 1, K_BSDF = 2, K_PHASE = 4, K_RR = 5, K_MEDIUM = 6, K_VOLUME = 7 };  // tracer.rs:23-30 (off vertex)
constexpr int kRrStartBounce = 3;                              // tracer.rs:46
constexpr float kRrMinProb = 0.05f;                            // tracer.rs:47

// What a vertex step leaves: the path's radiance and throughput behind the vertex, whether it goes on and, if so, the
// next ray (origin, direction, whether the sampled lobe was a delta); and what it adds to the six counters the shade
// kernels keep (closest_hit, vertices, roulette tests, roulette kills, escaped, ended at the depth limit — a vertex step
// never adds to `escaped`; the miss step does).
struct VertexOut {
  V3 origin, dir, beta, L;
  bool alive, delta;
  uint32_t closest, vertices, rr_tested, rr_killed, escaped, depth_ended;
};

// mat: the hit material's view (MatRaw / MatDerived). ro, rd: the ray that hit; rec: its hit (p = ray.at(t)). pattern,
// sample: the path sampler (K_PATH domain's pattern, sample index); n_rec: vertices recorded before this one; remaining:
// bounces left; prev_valid: the path has a previous vertex.
template <class MV>
__device__ __forceinline__ VertexOut vertex_simple(const MV &mat, V3 ro, V3 rd, V3 beta, V3 L, const HitRec &rec, uint32_t pattern,
                                                   uint32_t sample, uint32_t n_rec, int remaining, bool prev_valid,
                                                   const uint32_t *sobol_tab) {
  (void)ro;
  VertexOut o;
  o.origin = splat(0.0f); o.dir = splat(0.0f);
  o.alive = false; o.delta = false;
  o.closest = o.vertices = o.rr_tested = o.rr_killed = o.escaped = o.depth_ended = 0;
  const float emission_weight = 1.0f;  // bounce_emission_weight without lights (tracer.rs:930-953)
  if (remaining <= 0) {  // tracer.rs:1123-1149: depth exhausted, last-vertex emission only
    o.depth_ended = 1;
    if (prev_valid) {
      o.closest = 1;
      const float cos_o = fabs_(dot(normalize(rd), rec.normal));
      const V3 emitted = mat_emitted_directional<true>(mat, cos_o);
      if (len2(emitted) > 0.0f) L = L + beta * (emitted * emission_weight);
    }
  } else {
    o.closest = 1;
    const Sampler vdom = new_domain(Sampler{pattern, sample}, (int)n_rec);  // :1121
    const V3 atten = splat(1.0f);
    const float cos_o = fabs_(dot(normalize(rd), rec.normal));
    const V3 emitted = mat_emitted_directional<true>(mat, cos_o);
    V3 emit_here = splat(0.0f);
    if (prev_valid) {  // tracer.rs:1372-1381
      if (len2(emitted) > 0.0f) L = L + beta * ((atten * emitted) * emission_weight);
    } else {
      emit_here = emitted;
    }
    const V3 ba = beta * atten;
    L = L + ba * emit_here;
    // indirect lighting by BSDF sampling (tracer.rs:1459-1523)
    Scatter sample_s;
    if (mat_scatter<true>(mat, rd, rec, new_domain(vdom, K_BSDF), sample_s, sobol_tab)) {
      const V3 dir = normalize(sample_s.dir);
      const float cosine = sample_s.delta ? 1.0f : fabs_(dot(rec.normal, dir));
      const V3 factor = (sample_s.value * cosine) / sample_s.pdf;
      beta = beta * (atten * factor);
      bool survived = true;
      if (n_rec >= (uint32_t)kRrStartBounce) {
        o.rr_tested = 1;
        const float p_survive = rclamp(max_elem(beta), kRrMinProb, 1.0f);
        if (p_survive < 1.0f) {
          if (draw_rnd1(new_domain(vdom, K_RR)) >= p_survive) {
            survived = false;
            o.rr_killed = 1;
          } else {
            beta = beta / p_survive;
          }
        }
      }
      if (survived) {
        o.alive = true;
        o.origin = sample_s.origin; o.dir = sample_s.dir; o.delta = sample_s.delta;
      }
    }
    o.vertices = 1;
  }
  o.beta = beta;
  o.L = L;
  return o;
}

}  // namespace dev
}  // namespace crt
