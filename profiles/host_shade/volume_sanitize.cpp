// Stand-alone program (its own main) over the volume aggregate's host builder (csrc/volumes.cpp, volumes_build_image) and
// the walks of kernels/volume.hip.h compiled as host C++ behind the HIP stand-in header: every refusal of
// crt_volumes_new and the two walks that only the step bound ends, under AddressSanitizer + UndefinedBehaviorSanitizer
// on the CPU. Nothing here is loaded into Python and nothing runs on a GPU.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iprofiles/host_shade -Icrust-render_amd/csrc profiles/host_shade/volume_sanitize.cpp -o volume_sanitize
// The builder calls three functions of scene.cpp (affine_inverse, affine_point) and capi.cpp (set_error_text), files
// that need the HIP runtime; this program carries its own copies of those few lines, so it checks the builder's own
// code and the shared header, not those three.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#define CRT_VOLUMES_BUILDER_ONLY 1
#include "volumes.cpp"

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
static F3 mat3_mul(const Mat3 &m, F3 r) {
  F3 res = m.x * r.x;
  res = res + m.y * r.y;
  res = res + m.z * r.z;
  return res;
}
Mat3 mat3_transpose(const Mat3 &m) { return {f3(m.x.x, m.y.x, m.z.x), f3(m.x.y, m.y.y, m.z.y), f3(m.x.z, m.y.z, m.z.z)}; }
Affine affine_inverse(const Affine &a) {
  const F3 t0 = cross(a.y, a.z), t1 = cross(a.z, a.x), t2 = cross(a.x, a.y);
  const float inv = 1.0f / dot(a.z, t2);
  const Mat3 m = mat3_transpose(Mat3{t0 * inv, t1 * inv, t2 * inv});
  const F3 t = -mat3_mul(m, a.t);
  return {m.x, m.y, m.z, t};
}
F3 affine_point(const Affine &a, F3 p) { return mat3_mul(Mat3{a.x, a.y, a.z}, p) + a.t; }
}  // namespace crt

using namespace crt;
using namespace crt::dev;

static CrtVolumeRegion unit_region() {
  CrtVolumeRegion r;
  std::memset(&r, 0, sizeof(r));
  r.local_to_world[0] = r.local_to_world[4] = r.local_to_world[8] = 1.0f;
  for (int a = 0; a < 3; a++) { r.half_extent[a] = 0.5f; r.sigma_s[a] = 0.5f; }
  r.density_scale = 1.0f;
  r.noise_scale = 4.0f; r.noise_octaves = 4; r.noise_gain = 0.5f; r.noise_lacunarity = 2.0f; r.noise_threshold = 0.3f;
  return r;
}

static int refusals = 0, failures = 0;
static void expect_refused(const char *what, const CrtVolumeRegion *regs, size_t n, const float *grid, size_t grid_len) {
  std::vector<unsigned char> image;
  g_error.clear();
  const int rc = volumes_build_image(regs, n, grid, grid_len, image);
  if (rc != CRT_ERR_BAD_ARG || g_error.empty() || !image.empty()) { std::printf("NOT REFUSED: %s (rc %d, \"%s\")\n", what, rc, g_error.c_str()); failures++; }
  else refusals++;
}

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float grid8[8] = {0, 1, 2, 3, 4, 5, 6, 7};
  {
    CrtVolumeRegion nine[9];
    for (auto &r : nine) r = unit_region();
    expect_refused("nine regions", nine, 9, nullptr, 0);
    expect_refused("records missing", nullptr, 2, nullptr, 0);
    CrtVolumeRegion r = unit_region();
    r.sigma_a[1] = nan;
    expect_refused("NaN coefficient", &r, 1, nullptr, 0);
    r = unit_region(); r.local_to_world[10] = inf;
    expect_refused("infinite placement", &r, 1, nullptr, 0);
    r = unit_region(); r.noise_gain = nan;
    expect_refused("NaN noise parameter", &r, 1, nullptr, 0);
    r = unit_region(); r.field = 7;
    expect_refused("unknown field", &r, 1, nullptr, 0);
    r = unit_region(); r.field = CRT_VOLUME_NOISE; r.noise_octaves = 33;
    expect_refused("33 octaves", &r, 1, nullptr, 0);
    r = unit_region(); r.field = CRT_VOLUME_GRID; r.grid_dims[0] = 2; r.grid_dims[1] = 2; r.grid_dims[2] = 3; r.grid_count = 8;
    expect_refused("dims do not match", &r, 1, grid8, 8);
    r.grid_dims[2] = 0; r.grid_count = 0;
    expect_refused("dims multiply to 0", &r, 1, grid8, 8);
    r.grid_dims[0] = r.grid_dims[1] = r.grid_dims[2] = 0xffffffffu; r.grid_count = 8;
    expect_refused("dims overflow", &r, 1, grid8, 8);
    r.grid_dims[0] = r.grid_dims[1] = r.grid_dims[2] = 2; r.grid_count = 8; r.grid_offset = 1;
    expect_refused("offset outside", &r, 1, grid8, 8);
    r.grid_offset = 0;
    expect_refused("grid array missing", &r, 1, nullptr, 8);
    r = unit_region(); r.local_to_world[0] = 0.0f;
    expect_refused("singular placement", &r, 1, nullptr, 0);
  }
  // the walks only the bound ends: a pure-null-collision region (tests/volume_cases.py, step_limit_aggregate)
  int walks = 0;
  {
    CrtVolumeRegion r = unit_region();
    for (int a = 0; a < 3; a++) r.sigma_s[a] = 4.0f * CRT_VOLUME_MAX_STEPS;
    r.field = CRT_VOLUME_GRID; r.grid_dims[0] = r.grid_dims[1] = 1; r.grid_dims[2] = 4; r.grid_count = 4;
    const float grid[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    std::vector<unsigned char> image;
    if (volumes_build_image(&r, 1, grid, 4, image) != CRT_OK) { std::printf("the step-limit aggregate was refused: %s\n", g_error.c_str()); return 1; }
    const VolHeader *hd = reinterpret_cast<const VolHeader *>(image.data());
    const VolRegionRec *regs = reinterpret_cast<const VolRegionRec *>(image.data() + hd->off_regions);
    const float *g = reinterpret_cast<const float *>(image.data() + hd->off_grid);
    const V3 origins[2] = {v3(nan, nan, nan), v3(0.0f, 0.0f, -0.3f)}, dirs[2] = {v3(1.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f)};
    for (int k = 0; k < 2; k++) {
      float sa[kVolMaxRegions] = {}, sb[kVolMaxRegions] = {}, lw[kVolMaxRegions] = {};
      V3 tr;
      const uint32_t st = vol_transmittance(regs, hd->n_regions, g, origins[k], dirs[k], 1e-3f, inf, 99u + (uint32_t)k, sa, sb, 1, tr);
      const VolEvent E = vol_sample_interaction(regs, hd->n_regions, g, origins[k], dirs[k], 1e-3f, inf, 7u + (uint32_t)k, sa, sb, lw, 1);
      const bool ok = st == CRT_VOLUME_STEP_LIMIT && tr.x == 0.0f && tr.y == 0.0f && tr.z == 0.0f && E.status == CRT_VOLUME_STEP_LIMIT &&
                      E.kind == CRT_VOLUME_PASSTHROUGH && E.weight.x == 0.0f && E.weight.y == 0.0f && E.weight.z == 0.0f &&
                      E.emitted.x == 0.0f && E.n_lobes == 0u;
      if (!ok) { std::printf("walk %d did not end at the step limit (status %u / %u)\n", k, st, E.status); failures++; }
      walks += 2;
    }
  }
  std::printf("volume_sanitize: %d refusals, %d bounded walks, %d failures\n", refusals, walks, failures);
  return failures ? 1 : 0;
}
