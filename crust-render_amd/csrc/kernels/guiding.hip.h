// The path guiding field's device functions: crates/crust-core/src/guiding/{mod,dtree,sdtree,field}.rs restated in
// float32, one operation per reference operation, over the image csrc/guiding.cpp flattens the host field into. The SAME
// source runs in the seam kernels (kernels/guiding_seam.hip), in the library's host code (guiding.cpp records a training
// sample through guide_dir_to_canonical and guide_quadrant below) and in the tests' CPU twin (tests/host_shade/
// guiding_host.cpp). Compile with -ffp-contract=off (dmath.hip.h).
//
// The image (GuideHeader::bytes in one allocation, every array on a 256-byte boundary):
//   GuideHeader  256 bytes  magic, the padded bounds, alpha, array offsets and counts, the ACTUAL maximum depths
//   GuideSNode    16 bytes  axis (or kGuideLeaf), split, two children — or, in a leaf, its D-tree's root in `a`
//   GuideDNode    32 bytes  sums[4] then children[4], every D-tree in ONE array, children as indices into that array
// A lane fetches a D-node with two 16-byte loads that go out together. Nobody has measured whether this layout is
// better than a 16-byte sums-only node with implicit children; it is what upstream keeps, flattened.
//
// A kernel never dereferences a word a caller wrote: every index read from the image is range-checked against the
// header's counts before use, and a bad index ends the descent as "no information below" — it does not become a load.
// Both descents are `for` loops over the caps (CRT_GUIDING_MAX_*_DEPTH), tightened to the header's actual depths.
//
// Departures from upstream, all of them:
//   * cos / sin / atan2 are sincos_det / atan2_det (dmath.hip.h), not libm: the project's standing rule. Field bits are
//     therefore pinned device == restatement (tests/guiding_ref.py), and statistically against upstream's unit tests.
//   * normalize is the project's (a / sqrt(dot)), clamp of a position glam's max-then-min with SSE operand semantics
//     (vclamp); glam's own sources are not in the reference tree.
//   * (1 - z * z).max(0) is Rust's f32::max (a NaN operand yields the other one: rmax), f32::clamp passes a NaN
//     through (rclamp), `>=` on a NaN is false (a NaN takes quadrant 0).
//   * a D-tree's children are indices into the one shared array (root + upstream's index).
//   * the loops are bounded; upstream's `loop`s end because its trees are finite.
#pragma once

#include "dmath.hip.h"

namespace crt {
namespace dev {

constexpr uint32_t kGuideMagic = 0x44475243u;    // "CRGD"
constexpr uint32_t kGuideNoChild = 0xffffffffu;  // dtree.rs:14 NO_CHILD
constexpr uint32_t kGuideLeaf = 0xffffffffu;     // GuideSNode::axis of SNode::Leaf
constexpr uint32_t kGuideDTreeCap = 32u, kGuideSpatialCap = 32u;  // crt_guiding.h: CRT_GUIDING_MAX_*_DEPTH
#define CRT_GUIDE_ONE_MINUS_EPS 0.99999988079071044921875f  // dtree.rs:15: 1.0 - f32::EPSILON
#define CRT_GUIDE_TAU 6.28318530717958647692528676655900577f  // std::f32::consts::TAU
#define CRT_GUIDE_INV_4PI (1.0f / (4.0f * CRT_PI))             // dtree.rs:130, :172

struct GuideHeader {  // 256 bytes
  uint32_t magic, bytes;
  float bmin[3], bmax[3];  // the PADDED bounds (field.rs:63-72)
  float alpha;             // GuidingConfig::guide_prob
  uint32_t off_snodes, n_snodes, off_dnodes, n_dnodes, n_dtrees;
  uint32_t s_depth;        // the deepest spatial leaf (root = 0): a descent reads at most s_depth + 1 nodes
  uint32_t d_depth;        // the deepest D-tree (DTree::depth, a single root = 1): a descent reads at most d_depth nodes
  uint32_t pad[48];
};
struct alignas(16) GuideSNode { uint32_t axis; float split; uint32_t a, b; };
struct alignas(32) GuideDNode { float sums[4]; uint32_t children[4]; };
static_assert(sizeof(GuideHeader) == 256 && sizeof(GuideSNode) == 16 && sizeof(GuideDNode) == 32, "the image's records");

// What a kernel is handed: wave-uniform, so pointers, counts and bounds live in scalar registers.
struct GuideView {
  const GuideSNode *snodes;
  const GuideDNode *dnodes;
  uint32_t n_snodes, n_dnodes, s_depth, d_depth;
  float bmin[3], bmax[3];
  float alpha;
};

__device__ __forceinline__ float guide_sel4(float4 v, uint32_t q) { return q == 0 ? v.x : (q == 1 ? v.y : (q == 2 ? v.z : v.w)); }
__device__ __forceinline__ uint32_t guide_sel4(uint4 v, uint32_t q) { return q == 0 ? v.x : (q == 1 ? v.y : (q == 2 ? v.z : v.w)); }
__device__ __forceinline__ void guide_load_dnode(const GuideDNode *n, float4 &sums, uint4 &children) {
  sums = reinterpret_cast<const float4 *>(n)[0];
  children = reinterpret_cast<const uint4 *>(n)[1];
}
// DNode::total, dtree.rs:76-78
__device__ __forceinline__ float guide_total(float4 s) { return ((s.x + s.y) + s.z) + s.w; }

// guiding/mod.rs:18-20
__device__ __forceinline__ float guide_luminance(V3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// dtree.rs:19-27: a 64-bit LCG with an xorshift and a rotate; integer arithmetic only
__device__ __forceinline__ float guide_pcg_f32(uint64_t &state) {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  const uint32_t xorshifted = (uint32_t)(((state >> 18) ^ state) >> 27);
  const uint32_t rot = (uint32_t)(state >> 59);
  const uint32_t bits = (xorshifted >> rot) | (xorshifted << ((32u - rot) & 31u));
  return (float)(bits >> 8) * (1.0f / 16777216.0f);
}

// dtree.rs:30-35
__device__ __forceinline__ void guide_dir_to_canonical(V3 d, float p[2]) {
  d = normalize(d);
  const float u = atan2_det(d.y, d.x) / CRT_GUIDE_TAU + 0.5f;
  const float v = (d.z + 1.0f) * 0.5f;
  p[0] = rclamp(u, 0.0f, CRT_GUIDE_ONE_MINUS_EPS);
  p[1] = rclamp(v, 0.0f, CRT_GUIDE_ONE_MINUS_EPS);
}
// dtree.rs:38-43
__device__ __forceinline__ V3 guide_canonical_to_dir(const float p[2]) {
  const float phi = CRT_GUIDE_TAU * (p[0] - 0.5f);
  const float z = 2.0f * p[1] - 1.0f;
  const float r = sqrtf(rmax(1.0f - z * z, 0.0f));
  float s, c;
  sincos_det(phi, s, c);
  return v3(r * c, r * s, z);
}
// dtree.rs:48-56: the quadrant (qx + 2 * qy) and the point rescaled into it, in place
__device__ __forceinline__ uint32_t guide_quadrant(float p[2]) {
  const uint32_t qx = p[0] >= 0.5f ? 1u : 0u, qy = p[1] >= 0.5f ? 1u : 0u;
  p[0] = rclamp(p[0] * 2.0f - (float)qx, 0.0f, CRT_GUIDE_ONE_MINUS_EPS);
  p[1] = rclamp(p[1] * 2.0f - (float)qy, 0.0f, CRT_GUIDE_ONE_MINUS_EPS);
  return qx + 2u * qy;
}

// SDTree::leaf_index + dtree_at, sdtree.rs:43-66: the root node of the D-tree governing `pos`, or kGuideNoChild when the
// image does not lead to one (a bad index: no information)
__device__ __forceinline__ uint32_t guide_dtree_at(const GuideView &V, V3 pos) {
  const V3 p = vclamp(pos, v3(V.bmin[0], V.bmin[1], V.bmin[2]), v3(V.bmax[0], V.bmax[1], V.bmax[2]));
  const uint32_t levels = (V.s_depth < kGuideSpatialCap ? V.s_depth : kGuideSpatialCap) + 1u;
  uint32_t node = 0;
  for (uint32_t k = 0; k < levels; k++) {
    if (node >= V.n_snodes) return kGuideNoChild;
    const uint4 w = *reinterpret_cast<const uint4 *>(V.snodes + node);
    if (w.x == kGuideLeaf) return w.z < V.n_dnodes ? w.z : kGuideNoChild;
    if (w.x > 2u) return kGuideNoChild;
    node = comp(p, (int)w.x) >= __uint_as_float(w.y) ? w.w : w.z;
  }
  return kGuideNoChild;
}
// DTree::total_flux() > 0 of that tree: GuidingField::trained_at, field.rs:81-83
__device__ __forceinline__ bool guide_trained(const GuideView &V, uint32_t root) {
  if (root >= V.n_dnodes) return false;
  return guide_total(reinterpret_cast<const float4 *>(V.dnodes + root)[0]) > 0.0f;
}

// DTree::pdf, dtree.rs:125-151
__device__ __forceinline__ float guide_dtree_pdf(const GuideView &V, uint32_t root, float p[2]) {
  if (root >= V.n_dnodes) return 0.0f;
  const uint32_t levels = V.d_depth < kGuideDTreeCap ? V.d_depth : kGuideDTreeCap;
  uint32_t node = root;
  float pdf = CRT_GUIDE_INV_4PI;
  for (uint32_t k = 0; k < levels; k++) {
    float4 sums; uint4 children;
    guide_load_dnode(V.dnodes + node, sums, children);
    const float total = guide_total(sums);
    if (total <= 0.0f) return k == 0 ? 0.0f : pdf;  // an untrained tree: 0 | no information below: uniform over the domain
    const uint32_t q = guide_quadrant(p);
    const float frac = guide_sel4(sums, q) / total;
    if (frac <= 0.0f) return 0.0f;
    pdf *= 4.0f * frac;
    const uint32_t c = guide_sel4(children, q);
    if (c == kGuideNoChild || c >= V.n_dnodes) return pdf;
    node = c;
  }
  return pdf;
}

// DTree::sample, dtree.rs:163-219: false for None
__device__ __forceinline__ bool guide_dtree_sample(const GuideView &V, uint32_t root, float seed_u, float seed_v, float p[2], float &pdf_out) {
  if (root >= V.n_dnodes) return false;
  if (guide_total(reinterpret_cast<const float4 *>(V.dnodes + root)[0]) <= 0.0f) return false;  // total_flux() <= 0.0
  uint64_t rng = (((uint64_t)__float_as_uint(seed_u) << 32) | (uint64_t)__float_as_uint(seed_v)) ^ 0x9E3779B97F4A7C15ull;
  const uint32_t levels = V.d_depth < kGuideDTreeCap ? V.d_depth : kGuideDTreeCap;
  uint32_t node = root;
  float base0 = 0.0f, base1 = 0.0f, scale = 1.0f, pdf = CRT_GUIDE_INV_4PI;
  for (uint32_t k = 0; k < levels; k++) {
    float4 sums; uint4 children;
    guide_load_dnode(V.dnodes + node, sums, children);
    const float total = guide_total(sums);
    if (total <= 0.0f) break;  // no information below this node: uniform within its domain
    const float u0 = guide_pcg_f32(rng);
    const float u1 = guide_pcg_f32(rng);
    const float p_left = (sums.x + sums.z) / total;
    const uint32_t qx = u0 >= p_left ? 1u : 0u;
    const float col_total = (qx ? sums.y : sums.x) + (qx ? sums.w : sums.z);
    const float p_bottom = col_total > 0.0f ? (qx ? sums.y : sums.x) / col_total : 0.5f;
    const uint32_t qy = u1 >= p_bottom ? 1u : 0u;
    const uint32_t q = qx + 2u * qy;
    const float frac = guide_sel4(sums, q) / total;
    if (frac <= 0.0f) break;  // numerically unreachable quadrant: uninformative
    pdf *= 4.0f * frac;
    base0 += 0.5f * scale * (float)qx;
    base1 += 0.5f * scale * (float)qy;
    scale *= 0.5f;
    const uint32_t c = guide_sel4(children, q);
    if (c == kGuideNoChild || c >= V.n_dnodes) break;
    node = c;
  }
  const float u0 = guide_pcg_f32(rng);
  const float u1 = guide_pcg_f32(rng);
  p[0] = rclamp(base0 + u0 * scale, 0.0f, CRT_GUIDE_ONE_MINUS_EPS);
  p[1] = rclamp(base1 + u1 * scale, 0.0f, CRT_GUIDE_ONE_MINUS_EPS);
  pdf_out = pdf;
  return true;
}

// GuidingField::sample (field.rs:88-91) and ::pdf (field.rs:95-97) with trained_at beside them
__device__ __forceinline__ bool guide_field_sample(const GuideView &V, V3 pos, float seed_u, float seed_v, V3 &dir, float &pdf, bool &trained) {
  const uint32_t root = guide_dtree_at(V, pos);
  trained = guide_trained(V, root);
  float p[2];
  if (!guide_dtree_sample(V, root, seed_u, seed_v, p, pdf)) { dir = splat(0.0f); pdf = 0.0f; return false; }
  dir = guide_canonical_to_dir(p);
  return true;
}
// GuidingField::pdf behind the spatial descent: the D-tree `root` governs the position (shade_segment shares one descent
// between this and the bounce)
__device__ __forceinline__ float guide_field_pdf_at(const GuideView &V, uint32_t root, V3 dir) {
  float p[2];
  guide_dir_to_canonical(dir, p);
  return guide_dtree_pdf(V, root, p);
}
__device__ __forceinline__ float guide_field_pdf(const GuideView &V, V3 pos, V3 dir, bool &trained) {
  const uint32_t root = guide_dtree_at(V, pos);
  trained = guide_trained(V, root);
  return guide_field_pdf_at(V, root, dir);
}

}  // namespace dev
}  // namespace crt

// ---- the guided bounce: needs the shading functions (kernels/shade.hip.h) — included by whoever asks for it ----
#ifdef CRT_GUIDING_BOUNCE
#include "shade.hip.h"

namespace crt {
namespace dev {

constexpr int kDomainBsdf = 2, kDomainGuide = 3;  // tracer.rs: K_BSDF, K_GUIDE
constexpr uint32_t kGuidedTrained = 4u, kGuidedFromGuide = 8u;  // CrtScatterSample::flags bits 2 and 3

// Material::make_ray: openpbr.rs:1186-1200 — across a continuous-transmission interface the origin is p + wi * 1e-4 and
// the ray carries the interior only on the way in and only if the material has one; Emissive: material.rs:79-81.
// RESOLVE: the flag is checked against the material's interior here (the seam's answer); otherwise it says "enters through
// the front face" as mat_scatter's does, and the caller resolves it through its media table (shade_segment).
template <bool SIMPLE = false, bool RESOLVE = true>
__device__ __forceinline__ void guide_make_ray(const CrtMaterial &m, const HitRec &rec, V3 wi, V3 &origin, bool &medium) {
  origin = rec.p;
  medium = false;
  if (SIMPLE || m.kind == CRT_MAT_EMISSIVE) return;  // a simple-material table holds no transmission anywhere
  if (transmission_is_continuous(m) && dot(rec.normal, wi) < 0.0f) {
    origin = rec.p + wi * 1e-4f;
    if (rec.front_face) {
      medium = true;
      if (RESOLVE) {
        DevMedium med;
        medium_from_material(m, med);
        medium = med.present != 0;
      }
    }
  }
}
// Material::scatter_importance as the seam answers it (shade_seam.hip, k_seam_scatter): the medium flag only if the
// material has an interior (RESOLVE, as above)
template <bool SIMPLE = false, bool RESOLVE = true>
__device__ __forceinline__ bool guide_plain_scatter(const CrtMaterial &m, V3 rd, const HitRec &rec, Sampler dom, Scatter &sc, const uint32_t *tab) {
  const bool some = mat_scatter<SIMPLE>(m, rd, rec, dom, sc, tab);
  if (RESOLVE && some && sc.medium) {
    DevMedium med;
    medium_from_material(m, med);
    sc.medium = med.present != 0;
  }
  return some;
}

// sample_bounce_direction, tracer.rs:777-826, behind the spatial descent: `root` is guide_dtree_at(V, rec.p) and `trained`
// guide_trained(V, root) — the caller made them once and shares them with the NEE pdf (shade_segment), or just now
// (guide_sample_bounce below). v is the VERTEX domain. flags: kGuidedTrained | kGuidedFromGuide. One text for the seam
// kernel (RESOLVE) and the guided shade kernels (SIMPLE as the instance's): both read raw material records, the view
// every guided instance's table hands out (MatTable<false>: MatRaw).
// The text is the seam's as it stood, with its two mat_eval sites, so that the seam kernel keeps its registers and stays
// without scratch. A single-site form (one pass chooses wi, then evaluates; a second pass for the guide draw the material
// cannot evaluate) was compiled once while this was written and not kept: in the seam kernel the compiler then left mat_eval
// out of line (128 -> 153 VGPRs, 80 bytes of scratch). Whether it would shrink the guided shade instances is not known.
template <bool SIMPLE, bool RESOLVE>
__device__ __forceinline__ bool guide_sample_bounce_at(const GuideView &V, uint32_t root, bool trained, const CrtMaterial &m, V3 rd, const HitRec &rec,
                                                       Sampler v, Scatter &sc, uint32_t &flags, const uint32_t *tab) {
  const Sampler bsdf_dom = new_domain(v, kDomainBsdf);
  flags = 0;
  if (!trained) return guide_plain_scatter<SIMPLE, RESOLVE>(m, rd, rec, bsdf_dom, sc, tab);
  flags = kGuidedTrained;
  const float alpha = V.alpha;
  float gs[4];
  draw_sample4(new_domain(v, kDomainGuide), gs, tab);
  if (gs[0] < alpha) {
    // guide branch: draw from the field; the material's continuous component supplies the value and the BSDF pdf
    float p[2], p_guide;
    if (guide_dtree_sample(V, root, gs[1], gs[2], p, p_guide)) {
      const V3 wi = guide_canonical_to_dir(p);
      V3 value;
      float p_bsdf;
      if (mat_eval<SIMPLE>(m, rd, rec, wi, value, p_bsdf)) {
        sc.pdf = rmax(alpha * p_guide + (1.0f - alpha) * p_bsdf, 1e-4f);
        guide_make_ray<SIMPLE, RESOLVE>(m, rec, wi, sc.origin, sc.medium);
        sc.dir = wi;
        sc.value = value;
        sc.delta = false;
        flags |= kGuidedFromGuide;
        return true;
      }
    }
    return guide_plain_scatter<SIMPLE, RESOLVE>(m, rd, rec, bsdf_dom, sc, tab);  // no continuous component: pure BSDF sampling
  }
  if (!guide_plain_scatter<SIMPLE, RESOLVE>(m, rd, rec, bsdf_dom, sc, tab)) return false;
  if (sc.delta) {  // only this branch reaches the delta lobe: the coin scaled its selection probability by 1 - alpha
    sc.value = sc.value / (1.0f - alpha);
    return true;
  }
  const V3 wi = normalize(sc.dir);
  V3 value;
  float p_bsdf;
  if (mat_eval<SIMPLE>(m, rd, rec, wi, value, p_bsdf)) {
    float p[2];
    guide_dir_to_canonical(wi, p);
    const float p_guide = guide_dtree_pdf(V, root, p);
    sc.pdf = rmax(alpha * p_guide + (1.0f - alpha) * sc.pdf, 1e-4f);
  }
  return true;
}
// ... with its own descent: the seam's entry (kernels/guiding_seam.hip, tests/host_shade/guiding_host.cpp)
__device__ __forceinline__ bool guide_sample_bounce(const GuideView &V, const CrtMaterial &m, V3 rd, const HitRec &rec, Sampler v, Scatter &sc,
                                                    uint32_t &flags, const uint32_t *tab) {
  const uint32_t root = guide_dtree_at(V, rec.p);
  return guide_sample_bounce_at<false, true>(V, root, guide_trained(V, root), m, rd, rec, v, sc, flags, tab);
}

}  // namespace dev
}  // namespace crt
#endif  // CRT_GUIDING_BOUNCE
