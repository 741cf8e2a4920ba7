// Stand-alone program (its own main) over the per-face texture aggregate's host builder (csrc/face_textures.cpp,
// face_textures_build_image) and the two device functions of kernels/faces.hip.h compiled as host C++ behind the HIP
// stand-in header: every refusal of crt_face_textures_new, and resolve / eval over an image at the coordinates where an
// index could leave its table — exact 0 and 1, just outside, NaN, infinities, faces of one texel and of none, prim and
// face ids past their tables — under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU. Nothing here is loaded
// into Python and nothing runs on a GPU.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iprofiles/host_shade -Icrust-render_amd/csrc profiles/host_shade/face_textures_sanitize.cpp -o face_textures_sanitize
// The builder calls set_error_text (capi.cpp, a file that needs the HIP runtime); this program carries its own.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#define CRT_FACE_TEXTURES_BUILDER_ONLY 1
#include "face_textures.cpp"

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

using namespace crt;
using namespace crt::dev;

static int refusals = 0, failures = 0;

struct Inputs {
  std::vector<CrtFaceRect> rects{{0, 1, 1}, {1, 4, 2}, {9, 0, 3}, {9, 2, 0}, {9, 64, 16}};
  std::vector<float> texels = std::vector<float>(3 * (9 + 64 * 16), 0.25f);
  std::vector<uint32_t> faces{0, 0, 1, 4, 4, 7};
  std::vector<uint8_t> slices{1, 2, 0, 1, 3, 2};
  std::vector<CrtFaceBinding> bindings{{0, 0, 0}, {3, 0, 1}};
  std::vector<uint32_t> material_texture{0, CRT_INVALID_ID};
  CrtFaceTexture tex() const { return CrtFaceTexture{rects.data(), rects.size(), texels.data(), texels.size() / 3, {0.5f, 0.5f, 0.5f}}; }
  CrtFaceMap map() const { return CrtFaceMap{faces.data(), slices.data(), faces.size()}; }
  int build(std::vector<unsigned char> &image) const {
    const CrtFaceTexture t = tex();
    const CrtFaceMap m = map();
    return face_textures_build_image(&t, 1, &m, 1, bindings.data(), bindings.size(), material_texture.data(), material_texture.size(), image);
  }
};

static void expect_refused(const char *what, const Inputs &in) {
  std::vector<unsigned char> image;
  g_error.clear();
  if (in.build(image) == CRT_ERR_BAD_ARG && !g_error.empty() && image.empty()) { refusals++; return; }
  failures++;
  std::printf("NOT refused: %s\n", what);
}

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  { Inputs in; in.rects[1].offset = 1000000; expect_refused("a face past the texels", in); }
  { Inputs in; in.rects[1].offset = 0xffffffffu; expect_refused("an offset that wraps in 32 bits", in); }
  { Inputs in; in.rects[0].width = 16385; expect_refused("a face wider than the limit", in); }
  { Inputs in; in.slices[2] = 4; expect_refused("a slice above 3", in); }
  { Inputs in; in.texels[5] = nan; expect_refused("a NaN texel", in); }
  { Inputs in; in.texels[7] = -inf; expect_refused("an infinite texel", in); }
  { Inputs in; in.bindings[1].map = 1; expect_refused("a dangling map", in); }
  { Inputs in; in.bindings[1].geom_id = 0; expect_refused("a geometry bound twice", in); }
  { Inputs in; in.bindings[0].geom_id = CRT_FACE_MAX_GEOMS; expect_refused("a geometry past the limit", in); }
  { Inputs in; in.material_texture[1] = 1; expect_refused("a dangling texture", in); }
  {
    std::vector<unsigned char> image;
    const Inputs in;
    CrtFaceTexture t = in.tex();
    t.fallback[1] = inf;
    g_error.clear();
    if (face_textures_build_image(&t, 1, nullptr, 0, nullptr, 0, nullptr, 0, image) == CRT_ERR_BAD_ARG && !g_error.empty()) refusals++;
    else { failures++; std::printf("NOT refused: an infinite fallback\n"); }
    if (face_textures_build_image(nullptr, 1, nullptr, 0, nullptr, 0, nullptr, 0, image) == CRT_ERR_BAD_ARG) refusals++;
    else { failures++; std::printf("NOT refused: a NULL array\n"); }
  }

  // resolve and eval over a good image, at everything that could index outside it
  const Inputs in;
  std::vector<unsigned char> image;
  if (in.build(image) != CRT_OK) { std::printf("the good aggregate was refused: %s\n", g_error.c_str()); return 1; }
  FaceView F;
  face_view_of(image.data(), image.data(), F);
  const float edge[] = {0.0f, -0.0f, 1.0f, 0.99999994f, 1.0000001f, -1e-9f, 0.5f, 0.125f, 2.0f, -3.0f, 1e30f, -1e30f, nan, inf, -inf};
  const uint32_t ids[] = {0, 1, 2, 3, 4, 5, 6, 7, 1000, 0x7fffffffu, 0xfffffffeu, 0xffffffffu};
  long queries = 0;
  double sum = 0.0;
  for (uint32_t g : ids)
    for (uint32_t p : ids)
      for (float u : edge)
        for (float v : edge) {
          const FaceCoord c = face_resolve(F, g, p, u, v);
          if (c.u < 0.0f || c.u > 1.0f || c.v < 0.0f || c.v > 1.0f) failures++;  // f32::clamp: a NaN stays a NaN (eval reads it as 0)
          const V3 t = face_texture_eval(F, 0, c.face, c.u, c.v);
          sum += t.x;
          queries++;
        }
  for (uint32_t f : ids)
    for (float u : edge)
      for (float v : edge) {
        const V3 t = face_texture_eval(F, 0, f, u, v);
        // constant texels: any blend of them is 0.25 up to the rounding of (1 - s) + s; the fallback is 0.5
        if (!(std::fabs(t.x - 0.25f) < 1e-6f || t.x == 0.5f)) failures++;
        queries++;
      }
  std::printf("face_textures_sanitize: %d refusals, %ld queries, %d failures (%g)\n", refusals, queries, failures, sum);
  return failures ? 1 : 0;
}
