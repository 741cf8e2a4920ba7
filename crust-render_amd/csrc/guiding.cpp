// The path guiding field on the host: GuidingField (guiding/field.rs), SDTree (sdtree.rs) and DTree (dtree.rs) restated
// operation for operation — new with its padding, record, the two refines — plus the image the seam kernels read
// (kernels/guiding.hip.h: a 256-byte header, 16-byte spatial nodes, 32-byte directional nodes) and the handle's life.
// The host keeps what upstream keeps: S-nodes, a u64 sample_count per leaf, D-trees as node vectors; the counts never
// leave the host. Everything but the device copy at the end touches no device.
//
// Plain host C++ (the Makefile compiles this file with -x c++): a training sample is recorded through the device header's
// own guide_dir_to_canonical / guide_quadrant, compiled here for the host, so the host splat and a device descent agree
// bit for bit. CRT_GUIDING_HOST_ONLY (the stand-alone sanitizer program, profiles/host_shade/guiding_sanitize.cpp) drops
// the device copy and builds behind the HIP stand-in header.
//
// Departures from the reference, all named in DESIGN.md §2: the configuration is checked (crt_guiding_new), the depths
// are capped, and everything guiding.hip.h lists.
#include <atomic>
#include <cstring>
#include <new>

#ifndef CRT_GUIDING_HOST_ONLY
#include <hip/hip_runtime.h>
// the four bit casts the device headers use, which the HIP runtime header declares for device code only
static inline float __uint_as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline uint32_t __float_as_uint(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline double __longlong_as_double(long long v) { double d; std::memcpy(&d, &v, 8); return d; }
static inline long long __double_as_longlong(double d) { long long v; std::memcpy(&v, &d, 8); return v; }
#endif

#include "crt_internal.h"
#include "guiding_internal.h"

namespace crt {

using dev::GuideDNode;
using dev::GuideHeader;
using dev::GuideSNode;
using dev::kGuideLeaf;
using dev::kGuideNoChild;

namespace gfield {  // named: CrtGuiding below holds a Field

struct DTree {  // dtree.rs:83-85; a node is the image's record as it stands, children relative to this tree
  std::vector<GuideDNode> nodes;
  DTree() : nodes(1, leaf()) {}
  static GuideDNode leaf() { return GuideDNode{{0.0f, 0.0f, 0.0f, 0.0f}, {kGuideNoChild, kGuideNoChild, kGuideNoChild, kGuideNoChild}}; }
  static float total(const GuideDNode &n) { return ((n.sums[0] + n.sums[1]) + n.sums[2]) + n.sums[3]; }
  float total_flux() const { return total(nodes[0]); }

  // dtree.rs:106-121
  void record(float p[2], float flux) {
    if (!std::isfinite(flux) || flux <= 0.0f) return;
    size_t node = 0;
    for (;;) {
      const uint32_t q = dev::guide_quadrant(p);  // rescales p into the quadrant
      nodes[node].sums[q] += flux;
      const uint32_t c = nodes[node].children[q];
      if (c == kGuideNoChild) return;
      node = c;
    }
  }
  // dtree.rs:226-275
  DTree refine(float rho, uint32_t max_depth) const {
    DTree out;
    const float total = total_flux();
    if (total <= 0.0f) return out;
    refine_rec(out.nodes, 0, true, 0, nodes[0].sums, total, rho, 1, max_depth);
    return out;
  }
  void refine_rec(std::vector<GuideDNode> &out, size_t out_idx, bool has_old, size_t old_idx, const float seeded[4], float total, float rho,
                  uint32_t depth, uint32_t max_depth) const {
    float sums[4];
    for (int q = 0; q < 4; q++) sums[q] = has_old ? nodes[old_idx].sums[q] : seeded[q];
    for (int q = 0; q < 4; q++) out[out_idx].sums[q] = sums[q];
    for (int q = 0; q < 4; q++) {
      const float flux = sums[q];
      if (flux > rho * total && depth < max_depth) {
        const size_t child_idx = out.size();
        out.push_back(leaf());
        out[out_idx].children[q] = (uint32_t)child_idx;
        const uint32_t c = has_old ? nodes[old_idx].children[q] : kGuideNoChild;
        const float quarter = flux / 4.0f;
        const float seed[4] = {quarter, quarter, quarter, quarter};
        refine_rec(out, child_idx, c != kGuideNoChild, c, seed, total, rho, depth + 1, max_depth);
      }
    }
  }
  // dtree.rs:280-291
  uint32_t depth(size_t idx = 0) const {
    uint32_t d = 1;
    for (int q = 0; q < 4; q++)
      if (nodes[idx].children[q] != kGuideNoChild) { const uint32_t c = 1 + depth(nodes[idx].children[q]); d = c > d ? c : d; }
    return d;
  }
};

struct SNode {  // sdtree.rs:12-22
  bool leaf = true;
  uint32_t axis = 0; float split = 0.0f; uint32_t children[2] = {0, 0};  // Inner
  uint32_t dtree = 0; uint64_t sample_count = 0;                         // Leaf
};

struct Field {
  std::vector<SNode> nodes;
  std::vector<DTree> dtrees;
  F3 bmin{}, bmax{};  // padded
  CrtGuidingConfig cfg{};
  uint64_t recorded = 0;

  // sdtree.rs:43-58 (glam's clamp: max, then min, SSE operand semantics)
  size_t leaf_index(F3 p) const {
    p = vmin(vmax(p, bmin), bmax);
    size_t node = 0;
    while (!nodes[node].leaf) node = nodes[node].children[p[(int)nodes[node].axis] >= nodes[node].split ? 1 : 0];
    return node;
  }
  // sdtree.rs:70-80 behind field.rs:102-104
  void record(const CrtGuidingSample &s) {
    float canonical[2];
    dev::guide_dir_to_canonical(dev::v3(s.dir[0], s.dir[1], s.dir[2]), canonical);
    SNode &leaf = nodes[leaf_index(f3(s.pos[0], s.pos[1], s.pos[2]))];
    leaf.sample_count += 1;
    dtrees[leaf.dtree].record(canonical, s.radiance);
    recorded += 1;
  }
  // sdtree.rs:86-105
  void refine(uint32_t next_iteration) {
    // (spatial_c as f64 * 2.0f64.powi(next_iteration as i32).sqrt()).max(1.0) as u64 — `as` saturates, a NaN becomes 0;
    // f64::max answers the operand that is a number
    const double t = (double)cfg.spatial_c * std::sqrt(std::ldexp(1.0, (int)(int32_t)next_iteration));
    const double m = t > 1.0 ? t : 1.0;  // t.max(1.0): 1.0 unless t is the larger number (a NaN t: 1.0)
    const uint64_t threshold = m >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)m;
    split_rec(0, bmin, bmax, 0, threshold, cfg.spatial_max_depth);
    for (DTree &d : dtrees) d = d.refine(cfg.dtree_rho, cfg.dtree_max_depth);
    for (SNode &n : nodes)
      if (n.leaf) n.sample_count = 0;
  }
  // sdtree.rs:107-168
  void split_rec(size_t node, F3 lo, F3 hi, uint32_t depth, uint64_t threshold, uint32_t max_depth) {
    const SNode cur = nodes[node];
    if (!cur.leaf) {
      F3 max0 = hi, min1 = lo;
      max0.at((int)cur.axis) = cur.split; min1.at((int)cur.axis) = cur.split;
      split_rec(cur.children[0], lo, max0, depth + 1, threshold, max_depth);
      split_rec(cur.children[1], min1, hi, depth + 1, threshold, max_depth);
      return;
    }
    if (cur.sample_count <= threshold || depth >= max_depth) return;
    const F3 extent = hi - lo;
    const int axis = (extent.x >= extent.y && extent.x >= extent.z) ? 0 : (extent.y >= extent.z ? 1 : 2);
    const float split = 0.5f * (lo[axis] + hi[axis]);
    // both children start from the parent's distribution and half its sample statistic
    const uint32_t dtree1 = (uint32_t)dtrees.size();
    dtrees.push_back(DTree(dtrees[cur.dtree]));
    SNode a, b;
    a.dtree = cur.dtree; a.sample_count = cur.sample_count / 2;
    b.dtree = dtree1; b.sample_count = cur.sample_count / 2;
    const uint32_t c0 = (uint32_t)nodes.size();
    nodes.push_back(a);
    const uint32_t c1 = (uint32_t)nodes.size();
    nodes.push_back(b);
    SNode inner;
    inner.leaf = false; inner.axis = (uint32_t)axis; inner.split = split; inner.children[0] = c0; inner.children[1] = c1;
    nodes[node] = inner;
    F3 max0 = hi, min1 = lo;
    max0.at(axis) = split; min1.at(axis) = split;
    split_rec(c0, lo, max0, depth + 1, threshold, max_depth);
    split_rec(c1, min1, hi, depth + 1, threshold, max_depth);
  }

  uint32_t s_depth(size_t node = 0, uint32_t depth = 0) const {
    if (nodes[node].leaf) return depth;
    const uint32_t a = s_depth(nodes[node].children[0], depth + 1), b = s_depth(nodes[node].children[1], depth + 1);
    return a > b ? a : b;
  }
  void stats(CrtGuidingStats &st) const {
    st.s_nodes = (uint32_t)nodes.size();
    st.s_leaves = 0;
    for (const SNode &n : nodes) st.s_leaves += n.leaf ? 1u : 0u;
    st.s_depth = s_depth();
    st.d_trees = (uint32_t)dtrees.size();
    st.d_nodes = 0; st.d_depth = 0;
    for (const DTree &d : dtrees) {
      st.d_nodes += (uint32_t)d.nodes.size();
      const uint32_t k = d.depth();
      st.d_depth = k > st.d_depth ? k : st.d_depth;
    }
    st.recorded = recorded;
  }
  // The image: header | S-nodes | every D-tree in one array, each on a 256-byte boundary; a leaf names its D-tree's root
  // node, a D-node's children are indices into the shared array.
  int flatten(std::vector<unsigned char> &image) const {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    CrtGuidingStats st;
    stats(st);
    size_t n_d = 0;
    for (const DTree &d : dtrees) n_d += d.nodes.size();
    const size_t off_s = sizeof(GuideHeader), off_d = up(off_s + nodes.size() * sizeof(GuideSNode));
    const size_t bytes = up(off_d + n_d * sizeof(GuideDNode));
    if (n_d >= 0xffffffffull || bytes > 0xffffffffull) { set_error_text("crt_guiding_update: the image outgrew its 32-bit offsets"); return CRT_ERR_UNSUPPORTED; }
    image.assign(bytes, 0);
    GuideHeader hd;
    std::memset(&hd, 0, sizeof(hd));
    hd.magic = dev::kGuideMagic; hd.bytes = (uint32_t)bytes;
    for (int a = 0; a < 3; a++) { hd.bmin[a] = bmin[a]; hd.bmax[a] = bmax[a]; }
    hd.alpha = cfg.guide_prob;
    hd.off_snodes = (uint32_t)off_s; hd.n_snodes = (uint32_t)nodes.size();
    hd.off_dnodes = (uint32_t)off_d; hd.n_dnodes = (uint32_t)n_d; hd.n_dtrees = (uint32_t)dtrees.size();
    hd.s_depth = st.s_depth; hd.d_depth = st.d_depth;
    std::memcpy(image.data(), &hd, sizeof(hd));
    std::vector<uint32_t> roots(dtrees.size());
    GuideDNode *dn = reinterpret_cast<GuideDNode *>(image.data() + off_d);
    uint32_t at = 0;
    for (size_t t = 0; t < dtrees.size(); t++) {
      roots[t] = at;
      for (const GuideDNode &n : dtrees[t].nodes) {
        GuideDNode o = n;
        for (int q = 0; q < 4; q++)
          if (o.children[q] != kGuideNoChild) o.children[q] += roots[t];
        dn[at++] = o;
      }
    }
    GuideSNode *sn = reinterpret_cast<GuideSNode *>(image.data() + off_s);
    for (size_t i = 0; i < nodes.size(); i++) {
      const SNode &n = nodes[i];
      sn[i] = n.leaf ? GuideSNode{kGuideLeaf, 0.0f, roots[n.dtree], 0u} : GuideSNode{n.axis, n.split, n.children[0], n.children[1]};
    }
    return CRT_OK;
  }
};

}  // namespace gfield
}  // namespace crt

struct CrtGuiding {
  crt::gfield::Field field;
  std::vector<unsigned char> image;
  std::mutex mu;
  void *d_image = nullptr;  // uploaded on first device use
  bool stale = true;        // the image was rebuilt since the upload
  // the caller's reference and one per renderer the field is bound to (crt_renderer_set_guiding): crt_guiding_free drops
  // the caller's, the last one frees
  std::atomic<int> refs{1};
};

using namespace crt;
using namespace crt::gfield;

extern "C" {

void crt_guiding_config_default(CrtGuidingConfig *cfg) {
  if (!cfg) return;
  cfg->train_iterations = 4; cfg->guide_prob = 0.5f; cfg->spatial_c = 4000.0f; cfg->dtree_rho = 0.01f;
  cfg->dtree_max_depth = 20; cfg->spatial_max_depth = 24;
}

CrtGuiding *crt_guiding_new(const float bmin[3], const float bmax[3], const CrtGuidingConfig *cfg) {
  CrtGuiding *out = nullptr;
  (void)abi_guard("crt_guiding_new", [&] {
    if (!bmin || !bmax || !cfg) { set_error_text("crt_guiding_new: a NULL argument"); return (int)CRT_ERR_BAD_ARG; }
    for (int a = 0; a < 3; a++) {
      if (!std::isfinite(bmin[a]) || !std::isfinite(bmax[a])) { set_error_text("crt_guiding_new: the bounds are not finite"); return (int)CRT_ERR_BAD_ARG; }
      if (bmin[a] > bmax[a]) { set_error_text("crt_guiding_new: the bounds are inverted on axis %d", a); return (int)CRT_ERR_BAD_ARG; }
    }
    if (!std::isfinite(cfg->guide_prob) || !(cfg->guide_prob > 0.0f && cfg->guide_prob < 1.0f)) {
      set_error_text("crt_guiding_new: guide_prob %g is outside (0, 1)", (double)cfg->guide_prob);
      return (int)CRT_ERR_BAD_ARG;
    }
    if (!std::isfinite(cfg->spatial_c) || !(cfg->spatial_c > 0.0f)) { set_error_text("crt_guiding_new: spatial_c %g is not a positive number", (double)cfg->spatial_c); return (int)CRT_ERR_BAD_ARG; }
    if (!std::isfinite(cfg->dtree_rho) || !(cfg->dtree_rho > 0.0f)) { set_error_text("crt_guiding_new: dtree_rho %g is not a positive number", (double)cfg->dtree_rho); return (int)CRT_ERR_BAD_ARG; }
    if (cfg->dtree_rho < CRT_GUIDING_MIN_RHO) { set_error_text("crt_guiding_new: dtree_rho %g is below 1/1024", (double)cfg->dtree_rho); return (int)CRT_ERR_BAD_ARG; }
    if (cfg->dtree_max_depth == 0 || cfg->dtree_max_depth > CRT_GUIDING_MAX_DTREE_DEPTH) {
      set_error_text("crt_guiding_new: dtree_max_depth %u is outside 1 .. %u", cfg->dtree_max_depth, CRT_GUIDING_MAX_DTREE_DEPTH);
      return (int)CRT_ERR_BAD_ARG;
    }
    if (cfg->spatial_max_depth > CRT_GUIDING_MAX_SPATIAL_DEPTH) {
      set_error_text("crt_guiding_new: spatial_max_depth %u is above %u", cfg->spatial_max_depth, CRT_GUIDING_MAX_SPATIAL_DEPTH);
      return (int)CRT_ERR_BAD_ARG;
    }
    std::unique_ptr<CrtGuiding> g(new CrtGuiding());
    Field &f = g->field;
    // field.rs:66-67: pad the bounds so hit points exactly on the scene hull stay strictly inside
    const F3 lo = f3(bmin[0], bmin[1], bmin[2]), hi = f3(bmax[0], bmax[1], bmax[2]);
    const F3 ext = hi - lo;
    const float widest = sse_max(sse_max(ext.x, ext.y), ext.z) * 1e-3f;
    const float pad = (widest > 1e-3f) ? widest : 1e-3f;  // f32::max with a constant: the number
    f.bmin = lo - f3(pad, pad, pad);
    f.bmax = hi + f3(pad, pad, pad);
    f.cfg = *cfg;
    f.nodes.assign(1, SNode());
    f.dtrees.assign(1, DTree());
    const int rc = f.flatten(g->image);
    if (rc != CRT_OK) return rc;
    out = g.release();
    return (int)CRT_OK;
  });
  return out;
}

int crt_guiding_update(CrtGuiding *g, const CrtGuidingSample *host_samples, size_t n, uint32_t next_iteration) {
  if (!g || (n && !host_samples)) return CRT_ERR_BAD_ARG;
  return abi_guard("crt_guiding_update", [&] {
    std::lock_guard<std::mutex> lock(g->mu);
    Field next = g->field;  // all or nothing: a failed allocation leaves the field as it was
    for (size_t i = 0; i < n; i++) next.record(host_samples[i]);
    next.refine(next_iteration);
    std::vector<unsigned char> image;
    const int rc = next.flatten(image);
    if (rc != CRT_OK) return rc;
    g->field = std::move(next);
    g->image = std::move(image);
    g->stale = true;
    return (int)CRT_OK;
  });
}

int crt_guiding_image(const CrtGuiding *g, const void **image, size_t *bytes) {
  if (!g || !image || !bytes) return CRT_ERR_BAD_ARG;
  *image = g->image.data();
  *bytes = g->image.size();
  return CRT_OK;
}

int crt_guiding_stats(const CrtGuiding *g, CrtGuidingStats *out) {
  if (!g || !out) return CRT_ERR_BAD_ARG;
  g->field.stats(*out);
  return CRT_OK;
}

#ifdef CRT_GUIDING_HOST_ONLY
void crt_guiding_free(CrtGuiding *g) { delete g; }
#else
void crt_guiding_free(CrtGuiding *g) { guiding_release(g); }
#endif

}  // extern "C"

#ifndef CRT_GUIDING_HOST_ONLY
namespace crt {

void guiding_retain(CrtGuiding *g) { if (g) g->refs.fetch_add(1, std::memory_order_relaxed); }
void guiding_release(CrtGuiding *g) {
  if (!g || g->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  if (g->d_image) {
    (void)hipDeviceSynchronize();  // nothing that was handed the image may still be reading it
    (void)hipFree(g->d_image);
  }
  delete g;
}

int guiding_device(CrtGuiding *g, dev::GuideView &out) {
  std::lock_guard<std::mutex> lock(g->mu);
  if (g->stale) {
    if (!device_ok()) return CRT_ERR_NO_DEVICE;
    if (g->d_image) {
      if (!CRT_HIP_OK(hipDeviceSynchronize())) return CRT_ERR_NO_DEVICE;  // launches handed the old image have finished
      (void)hipFree(g->d_image);
      g->d_image = nullptr;
    }
    void *d = nullptr;
    if (!CRT_HIP_OK(hipMalloc(&d, g->image.size()))) return CRT_ERR_NO_DEVICE;
    if (!CRT_HIP_OK(hipMemcpy(d, g->image.data(), g->image.size(), hipMemcpyHostToDevice))) { (void)hipFree(d); return CRT_ERR_NO_DEVICE; }
    g->d_image = d;
    g->stale = false;
  }
  const GuideHeader *hd = reinterpret_cast<const GuideHeader *>(g->image.data());
  const unsigned char *base = static_cast<const unsigned char *>(g->d_image);
  out.snodes = reinterpret_cast<const GuideSNode *>(base + hd->off_snodes);
  out.dnodes = reinterpret_cast<const GuideDNode *>(base + hd->off_dnodes);
  out.n_snodes = hd->n_snodes; out.n_dnodes = hd->n_dnodes;
  out.s_depth = hd->s_depth; out.d_depth = hd->d_depth;
  for (int a = 0; a < 3; a++) { out.bmin[a] = hd->bmin[a]; out.bmax[a] = hd->bmax[a]; }
  out.alpha = hd->alpha;
  return CRT_OK;
}

}  // namespace crt
#endif
