// Stand-alone program (its own main) over the guiding field's host code (csrc/guiding.cpp: new / update / refine /
// flatten) and the descents of kernels/guiding.hip.h compiled as host C++ behind the HIP stand-in header: the one_point,
// deep_spatial and zero_flux recipes of tests/guiding_cases.py, every refusal of crt_guiding_new, and sample / pdf on a
// hand-made query list (positions beyond the bounds, infinite and NaN; zero, NaN and unnormalised directions; seeds 0,
// 1 - 2^-24, NaN) — under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU. Nothing here is loaded into Python
// and nothing runs on a GPU.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iprofiles/host_shade -Icrust-render_amd/csrc profiles/host_shade/guiding_sanitize.cpp -o guiding_sanitize
// guiding.cpp calls set_error_text of capi.cpp, a file that needs the HIP runtime; this program carries its own.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#define CRT_GUIDING_HOST_ONLY 1
#include "guiding.cpp"

namespace crt {
static std::string g_error;
void set_error_text(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
}
}  // namespace crt

using namespace crt::dev;

static int refusals = 0, failures = 0, fields = 0;
static size_t queries = 0;
static const float kLo[3] = {-5.0f, -5.0f, -5.0f}, kHi[3] = {5.0f, 5.0f, 5.0f};

static void expect_refused(const char *what, const float *lo, const float *hi, const CrtGuidingConfig *cfg) {
  crt::g_error.clear();
  CrtGuiding *g = crt_guiding_new(lo, hi, cfg);
  if (g || crt::g_error.empty()) { std::printf("NOT refused: %s\n", what); failures++; }
  crt_guiding_free(g);
  refusals++;
}

static uint64_t lcg = 0x2545F4914F6CDD1Dull;
static float rnd() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (float)(lcg >> 40) * (1.0f / 16777216.0f); }

static GuideView view_of(const CrtGuiding *g) {
  const void *image = nullptr;
  size_t bytes = 0;
  if (crt_guiding_image(g, &image, &bytes) != CRT_OK || bytes < sizeof(GuideHeader)) { failures++; std::printf("no image\n"); }
  const unsigned char *im = static_cast<const unsigned char *>(image);
  GuideHeader h;
  std::memcpy(&h, im, sizeof(h));
  if (h.magic != kGuideMagic || h.bytes != bytes || h.off_dnodes + (size_t)h.n_dnodes * sizeof(GuideDNode) > bytes) { failures++; std::printf("bad header\n"); }
  GuideView V;
  V.snodes = reinterpret_cast<const GuideSNode *>(im + h.off_snodes);
  V.dnodes = reinterpret_cast<const GuideDNode *>(im + h.off_dnodes);
  V.n_snodes = h.n_snodes; V.n_dnodes = h.n_dnodes; V.s_depth = h.s_depth; V.d_depth = h.d_depth;
  for (int a = 0; a < 3; a++) { V.bmin[a] = h.bmin[a]; V.bmax[a] = h.bmax[a]; }
  V.alpha = h.alpha;
  return V;
}

// sample and pdf over the hand-made list; every call returns (the loops are bounded) and a pdf is never negative
static void descend(const CrtGuiding *g) {
  const GuideView V = view_of(g);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float pos[][3] = {{0, 0, 0}, {-5, -5, -5}, {5.01f, 5.01f, 5.01f}, {-7, 0, 9}, {1e30f, -1e30f, 0}, {inf, 0, 0}, {-inf, inf, 1},
                          {nan, 0, 0}, {nan, nan, nan}, {1.25f, -2.5f, 3.75f}, {2.5f, -1.0f, 3.0f}};
  const float dir[][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 0, 1}, {0, 0, -1}, {0, 0, 0}, {nan, 0, 1}, {3, -4, 12}, {inf, 1, 0}, {-1, -0.0f, 0}, {0.3f, -0.5f, 0.8f}};
  const float seed[] = {0.0f, 1.0f - 5.9604645e-8f, 0.5f, nan};
  for (const auto &p : pos)
    for (const auto &d : dir)
      for (float su : seed)
        for (float sv : seed) {
          V3 out; float pdf; bool trained;
          const bool some = guide_field_sample(V, v3(p[0], p[1], p[2]), su, sv, out, pdf, trained);
          if (some && !(pdf > 0.0f)) { failures++; std::printf("a sample without a positive pdf\n"); }
          const float q = guide_field_pdf(V, v3(p[0], p[1], p[2]), v3(d[0], d[1], d[2]), trained);
          if (q < 0.0f) { failures++; std::printf("a negative pdf\n"); }
          queries += 2;
        }
}

static void run_field(const char *what, const CrtGuidingConfig &cfg, int passes, size_t n, int recipe, uint32_t want_s, uint32_t want_d) {
  CrtGuiding *g = crt_guiding_new(kLo, kHi, &cfg);
  if (!g) { std::printf("%s: refused: %s\n", what, crt::g_error.c_str()); failures++; return; }
  descend(g);  // the untrained field
  std::vector<CrtGuidingSample> s(n);
  for (int k = 0; k < passes; k++) {
    for (size_t i = 0; i < n; i++) {
      CrtGuidingSample &o = s[i];
      std::memset(&o, 0, sizeof(o));
      if (recipe == 0) {  // one_point
        o.pos[0] = 1.25f; o.pos[1] = -2.5f; o.pos[2] = 3.75f; o.dir[0] = 0.3f; o.dir[1] = -0.5f; o.dir[2] = 0.8f; o.radiance = 1.0f;
      } else if (recipe == 1) {  // deep_spatial: two clusters
        const float *c = (i & 1) ? kLo : kHi;
        for (int a = 0; a < 3; a++) { o.pos[a] = 0.5f * c[a] + (rnd() - 0.5f); o.dir[a] = rnd() + 0.01f; }
        o.radiance = 0.1f + 3.0f * rnd();
      } else {  // zero_flux: counted, never splat
        for (int a = 0; a < 3; a++) { o.pos[a] = 10.0f * rnd() - 5.0f; o.dir[a] = rnd() - 0.5f; }
        o.radiance = (i % 3) == 0 ? 0.0f : ((i % 3) == 1 ? std::numeric_limits<float>::quiet_NaN() : -1.0f);
      }
    }
    if (crt_guiding_update(g, s.data(), n, (uint32_t)(k + 1)) != CRT_OK) { failures++; std::printf("%s: update failed\n", what); }
    descend(g);
  }
  CrtGuidingStats st;
  if (crt_guiding_stats(g, &st) != CRT_OK || st.recorded != (uint64_t)passes * n) { failures++; std::printf("%s: tallies\n", what); }
  if ((want_s && st.s_depth != want_s) || (want_d && st.d_depth != want_d) || (recipe == 2 && (st.d_nodes != st.d_trees || st.s_leaves < 2))) {
    failures++;
    std::printf("%s: depths %u %u, %u nodes in %u trees\n", what, st.s_depth, st.d_depth, st.d_nodes, st.d_trees);
  }
  if (crt_guiding_update(g, nullptr, 0, 9) != CRT_OK || crt_guiding_update(g, nullptr, 3, 9) != CRT_ERR_BAD_ARG) { failures++; std::printf("%s: empty pass\n", what); }
  crt_guiding_free(g);
  fields++;
}

int main() {
  CrtGuidingConfig def;
  crt_guiding_config_default(&def);
  if (def.train_iterations != 4 || def.guide_prob != 0.5f || def.spatial_c != 4000.0f || def.dtree_rho != 0.01f || def.dtree_max_depth != 20 ||
      def.spatial_max_depth != 24) { failures++; std::printf("defaults\n"); }
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float bad_lo[3] = {-5.0f, nan, -5.0f}, bad_hi[3] = {5.0f, inf, 5.0f}, inv_hi[3] = {5.0f, -6.0f, 5.0f};
  expect_refused("NaN bounds", bad_lo, kHi, &def);
  expect_refused("infinite bounds", kLo, bad_hi, &def);
  expect_refused("inverted bounds", kLo, inv_hi, &def);
  expect_refused("no bounds", nullptr, kHi, &def);
  expect_refused("no config", kLo, kHi, nullptr);
  CrtGuidingConfig c;
  for (float a : {0.0f, 1.0f, -0.5f, 1.5f, nan, inf}) { c = def; c.guide_prob = a; expect_refused("guide_prob", kLo, kHi, &c); }
  for (float v : {0.0f, -1.0f, nan, inf}) { c = def; c.spatial_c = v; expect_refused("spatial_c", kLo, kHi, &c); }
  for (float v : {0.0f, -0.01f, nan, inf, 1.0f / 2048.0f}) { c = def; c.dtree_rho = v; expect_refused("dtree_rho", kLo, kHi, &c); }
  for (uint32_t v : {0u, 33u, 0xffffffffu}) { c = def; c.dtree_max_depth = v; expect_refused("dtree_max_depth", kLo, kHi, &c); }
  for (uint32_t v : {33u, 0xffffffffu}) { c = def; c.spatial_max_depth = v; expect_refused("spatial_max_depth", kLo, kHi, &c); }
  crt_guiding_free(nullptr);

  c = def; c.spatial_c = 4.0f; c.spatial_max_depth = 5; c.dtree_max_depth = 8;
  run_field("one_point", c, 4, 2000, 0, 5, 8);
  c = def; c.spatial_c = 4.0f; c.spatial_max_depth = 32; c.dtree_max_depth = 32; c.dtree_rho = CRT_GUIDING_MIN_RHO;  // the caps themselves
  run_field("one_point at the caps", c, 12, 4000, 0, 0, 32);
  c = def; c.spatial_c = 4.0f;
  run_field("deep_spatial", c, 5, 600, 1, 0, 0);
  c = def; c.spatial_c = 16.0f;
  run_field("zero_flux", c, 2, 900, 2, 0, 0);
  c = def; c.spatial_max_depth = 0; c.spatial_c = 1.0f;  // a spatial tree that may never split
  run_field("no spatial split", c, 2, 500, 1, 0, 0);

  std::printf("guiding_sanitize: %d refusals, %d fields, %zu descents, %d failures\n", refusals, fields, queries, failures);
  return failures == 0 ? 0 : 1;
}
