// The environment object of a mapped dome light: the reference's Distribution1D::new and EnvironmentMap::new
// (environment.rs:39-66, :120-144) restated operation for operation on the host, the image the kernels read
// (kernels/envmap.hip.h) and the library's table of live environments.
//
// Departures from the reference, all named in DESIGN.md §2:
//   * sin(theta) of a row comes from sincos_det — the device's own function compiled for the host, as flat_tri_normal is
//     shared — not from libm's sinf. No vendor sinf / atan2f is on this path.
//   * a non-finite texel (and a luminance weight that overflows f32) is REFUSED; the reference accepts it and poisons
//     its CDF. Negative texels are accepted as upstream: weight 0, radiance as authored.
//   * a light_to_world without an inverse is refused (glam asserts in debug builds and returns infinities otherwise).
// Building touches no device, as commit() touches none: the image is uploaded on first device use.
#include <cstdarg>
#include <cstring>
#include <new>

#include "crt_internal.h"
#include "kernels/envmap.hip.h"

namespace crt {

using dev::EnvHeader;
using dev::EnvSlot;
using dev::kEnvSlots;

static inline float rust_max(float a, float b) { return (a > b || b != b) ? a : b; }  // f32::max

// Distribution1D::new (environment.rs:40-66): cdf has n + 1 entries.
static float distribution1d(const float *func, size_t n, float *cdf) {
  cdf[0] = 0.0f;
  double running = 0.0;
  for (size_t i = 0; i < n; i++) {
    running += (double)func[i] / (double)n;
    cdf[i + 1] = (float)running;
  }
  const float integral = (float)running;
  if (integral > 0.0f) {
    for (size_t i = 0; i <= n; i++) cdf[i] /= integral;
  } else {
    for (size_t i = 0; i <= n; i++) cdf[i] = (float)i / (float)n;
  }
  return integral;
}

static uint32_t bisect_steps(uint32_t n) {  // ceil(log2(n + 1))
  uint32_t s = 0;
  while (((uint64_t)1 << s) < (uint64_t)n + 1u) s++;
  return s;
}

// glam Mat3A::inverse: three cross products, det = z . (x cross y), times 1 / det, transposed. Columns x, y, z.
static bool mat3_inverse(const float m[9], float out[9]) {
  const F3 x = f3(m[0], m[1], m[2]), y = f3(m[3], m[4], m[5]), z = f3(m[6], m[7], m[8]);
  const F3 t0 = cross(y, z), t1 = cross(z, x), t2 = cross(x, y);
  const float det = dot(z, t2);
  const float inv = 1.0f / det;
  const F3 c0 = t0 * inv, c1 = t1 * inv, c2 = t2 * inv;
  const float r[9] = {c0.x, c1.x, c2.x, c0.y, c1.y, c2.y, c0.z, c1.z, c2.z};  // transpose
  bool ok = det != 0.0f;
  for (int i = 0; i < 9; i++) { out[i] = r[i]; ok = ok && std::isfinite(r[i]); }
  return ok;
}

struct Environment {
  uint32_t w = 0, h = 0, id = 0;
  std::vector<float> marg_func, marg_cdf, cond_func, cond_cdf, cond_integral;
  float marg_integral = 0.0f;
  float l2w[9], w2l[9];
  std::vector<unsigned char> image;  // the device image, built on the host
  void *d_image = nullptr;           // uploaded on first device use (env_mu)
  ~Environment();
};

// The table of live environments: kEnvSlots slots, id = generation << 4 | slot. The host half lives here; the device
// half (kEnvSlots EnvSlot records, allocated with the first upload) is what the library's own launches hand to the kernels.
static std::mutex env_mu;
static Environment *env_live[kEnvSlots];
static uint32_t env_generation[kEnvSlots];
static EnvSlot *d_env_table = nullptr;

static bool write_slot(uint32_t slot, const void *image, uint32_t generation) {
  EnvSlot s{static_cast<const EnvHeader *>(image), generation, 0u};
  return CRT_HIP_OK(hipMemcpy(d_env_table + slot, &s, sizeof(EnvSlot), hipMemcpyHostToDevice));
}

Environment::~Environment() {
  if (id == 0) return;
  std::lock_guard<std::mutex> lock(env_mu);
  const uint32_t slot = id & (kEnvSlots - 1u);
  env_live[slot] = nullptr;
  if (d_image) {
    (void)hipDeviceSynchronize();  // nothing that was handed the table may still be reading the image
    (void)write_slot(slot, nullptr, 0u);
    (void)hipFree(d_image);
  }
}

static int upload_locked(Environment &e) {
  if (e.d_image) return CRT_OK;
  if (!device_ok()) return CRT_ERR_NO_DEVICE;
  if (!d_env_table) {
    if (!CRT_HIP_OK(hipMalloc(&d_env_table, kEnvSlots * sizeof(EnvSlot)))) { d_env_table = nullptr; return CRT_ERR_NO_DEVICE; }
    if (!CRT_HIP_OK(hipMemset(d_env_table, 0, kEnvSlots * sizeof(EnvSlot)))) return CRT_ERR_NO_DEVICE;
  }
  void *d = nullptr;
  if (!CRT_HIP_OK(hipMalloc(&d, e.image.size()))) return CRT_ERR_NO_DEVICE;
  if (!CRT_HIP_OK(hipMemcpy(d, e.image.data(), e.image.size(), hipMemcpyHostToDevice)) ||
      !write_slot(e.id & (kEnvSlots - 1u), d, e.id >> 4)) {
    (void)hipFree(d);
    return CRT_ERR_NO_DEVICE;
  }
  e.d_image = d;
  return CRT_OK;
}

// The device table for a launch of the library's own: every live environment uploaded. *table = nullptr when none is
// live (the launch then takes the instance without the mapped arm).
int env_table_for_launch(const void **table) {
  std::lock_guard<std::mutex> lock(env_mu);
  *table = nullptr;
  bool any = false;
  for (uint32_t s = 0; s < kEnvSlots; s++) {
    if (!env_live[s]) continue;
    const int rc = upload_locked(*env_live[s]);
    if (rc != CRT_OK) return rc;
    any = true;
  }
  if (any) *table = d_env_table;
  return CRT_OK;
}

}  // namespace crt

struct CrtEnvironment { std::shared_ptr<crt::Environment> p; };

namespace crt {

static std::weak_ptr<Environment> env_weak[kEnvSlots];

// A reference to the environment a light record names (a renderer retains what its lights name, as it retains its
// scene), or nothing when the id is out of range, freed or of an older generation.
std::shared_ptr<void> env_retain(uint32_t id) {
  std::lock_guard<std::mutex> lock(env_mu);
  const uint32_t slot = id & (kEnvSlots - 1u);
  if ((id >> 4) == 0u || !env_live[slot] || env_live[slot]->id != id) return nullptr;
  return env_weak[slot].lock();
}

}  // namespace crt

using namespace crt;

extern "C" {

CrtEnvironment *crt_environment_new(uint32_t width, uint32_t height, const float *rgb, const float light_to_world[9]) {
  CrtEnvironment *out = nullptr;
  (void)abi_guard("crt_environment_new", [&] {
    if (width == 0 || height == 0 || width > 16384u || height > 16384u) {
      set_error_text("crt_environment_new: a %u x %u map (each side must be 1 .. 16384)", width, height);
      return (int)CRT_ERR_BAD_ARG;
    }
    if (!rgb) { set_error_text("crt_environment_new: no pixels"); return (int)CRT_ERR_BAD_ARG; }
    const size_t w = width, h = height;
    for (size_t k = 0; k < w * h * 3; k++)
      if (!std::isfinite(rgb[k])) {
        set_error_text("crt_environment_new: texel (%zu, %zu) is not finite", (k / 3) % w, (k / 3) / w);
        return (int)CRT_ERR_BAD_ARG;
      }
    auto e = std::make_shared<Environment>();
    e->w = width; e->h = height;
    static const float identity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::memcpy(e->l2w, light_to_world ? light_to_world : identity, sizeof(e->l2w));
    bool finite = true;
    for (int i = 0; i < 9; i++) finite = finite && std::isfinite(e->l2w[i]);
    if (!finite || !mat3_inverse(e->l2w, e->w2l)) {
      set_error_text("crt_environment_new: light_to_world has no finite inverse");
      return (int)CRT_ERR_BAD_ARG;
    }
    e->cond_func.resize(w * h); e->cond_cdf.resize(h * (w + 1)); e->cond_integral.resize(h);
    e->marg_func.resize(h); e->marg_cdf.resize(h + 1);
    for (size_t y = 0; y < h; y++) {  // environment.rs:126-136
      const float theta = ((float)y + 0.5f) / (float)h * CRT_PI;
      float sin_theta, cos_theta;
      dev::sincos_det(theta, sin_theta, cos_theta);
      float *row = &e->cond_func[y * w];
      for (size_t x = 0; x < w; x++) {
        const float *c = rgb + 3 * (y * w + x);
        const float lum = 0.2126f * c[0] + 0.7152f * c[1] + 0.0722f * c[2];
        row[x] = rust_max(lum, 0.0f) * sin_theta;
        if (!std::isfinite(row[x])) {
          set_error_text("crt_environment_new: the luminance of texel (%zu, %zu) overflows", x, y);
          return (int)CRT_ERR_BAD_ARG;
        }
      }
      e->cond_integral[y] = distribution1d(row, w, &e->cond_cdf[y * (w + 1)]);
      e->marg_func[y] = e->cond_integral[y];
    }
    e->marg_integral = distribution1d(e->marg_func.data(), h, e->marg_cdf.data());
    // the image
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    EnvHeader hd;
    std::memset(&hd, 0, sizeof(hd));
    hd.w = width; hd.h = height; hd.marg_integral = e->marg_integral;
    hd.steps_w = bisect_steps(width); hd.steps_h = bisect_steps(height);
    size_t off = sizeof(EnvHeader);
    hd.off_texels = (uint32_t)off; off = up(off + w * h * 16);
    hd.off_rows = (uint32_t)off; off = up(off + h * 8);
    hd.off_ccdf = (uint32_t)off; off = up(off + h * (w + 1) * 4);
    hd.off_mcdf = (uint32_t)off; off = up(off + (h + 1) * 4);
    hd.bytes = (uint32_t)off;  // offsets are 32-bit: the largest maps (16384 x 16384 needs 5.4 GB) are refused here
    if (off > 0xffffffffull) { set_error_text("crt_environment_new: a %u x %u map needs an image above 4 GiB", width, height); return (int)CRT_ERR_BAD_ARG; }
    std::memcpy(hd.l2w, e->l2w, sizeof(hd.l2w));
    std::memcpy(hd.w2l, e->w2l, sizeof(hd.w2l));
    e->image.assign(off, 0);
    unsigned char *im = e->image.data();
    std::memcpy(im, &hd, sizeof(hd));
    float *tex = reinterpret_cast<float *>(im + hd.off_texels);
    for (size_t k = 0; k < w * h; k++) { tex[4 * k] = rgb[3 * k]; tex[4 * k + 1] = rgb[3 * k + 1]; tex[4 * k + 2] = rgb[3 * k + 2]; tex[4 * k + 3] = e->cond_func[k]; }
    float *rows = reinterpret_cast<float *>(im + hd.off_rows);
    for (size_t y = 0; y < h; y++) { rows[2 * y] = e->cond_integral[y]; rows[2 * y + 1] = e->marg_func[y]; }
    std::memcpy(im + hd.off_ccdf, e->cond_cdf.data(), h * (w + 1) * 4);
    std::memcpy(im + hd.off_mcdf, e->marg_cdf.data(), (h + 1) * 4);
    // a slot and an id
    CrtEnvironment *handle = new CrtEnvironment();
    {
      std::lock_guard<std::mutex> lock(env_mu);
      uint32_t slot = kEnvSlots;
      for (uint32_t s = 0; s < kEnvSlots && slot == kEnvSlots; s++) if (!env_live[s]) slot = s;
      if (slot == kEnvSlots) {
        delete handle;
        set_error_text("crt_environment_new: all %u environment slots are in use", kEnvSlots);
        return (int)CRT_ERR_BAD_ARG;
      }
      // Generations run 0x00080000 .. 0x07f7ffff, so that the id's bits are a NORMAL finite float (0x00800000 <= id <
      // 0x7f800000): neither flushed to zero nor quieted where a host moves the record's fields as floats (crt.h).
      env_generation[slot] = (env_generation[slot] < 0x00080000u || env_generation[slot] >= 0x07f7ffffu)
                                 ? 0x00080000u : env_generation[slot] + 1u;
      e->id = env_generation[slot] << 4 | slot;
      env_live[slot] = e.get();
      env_weak[slot] = e;
    }
    handle->p = std::move(e);
    out = handle;
    return (int)CRT_OK;
  });
  return out;
}

void crt_environment_free(CrtEnvironment *env) { delete env; }

int crt_environment_tables(const CrtEnvironment *env, CrtEnvironmentTables *out) {
  if (!env || !out) return CRT_ERR_BAD_ARG;
  const Environment &e = *env->p;
  std::memset(out, 0, sizeof(*out));
  out->width = e.w; out->height = e.h; out->id = e.id;
  out->marginal_integral = e.marg_integral;
  out->marginal_func = e.marg_func.data(); out->marginal_cdf = e.marg_cdf.data();
  out->conditional_func = e.cond_func.data(); out->conditional_cdf = e.cond_cdf.data();
  out->conditional_integral = e.cond_integral.data();
  std::memcpy(out->light_to_world, e.l2w, sizeof(e.l2w));
  std::memcpy(out->world_to_light, e.w2l, sizeof(e.w2l));
  out->image = e.image.data(); out->image_bytes = e.image.size();
  return CRT_OK;
}

int crt_light_dome_mapped(CrtLight *out, const float tint[3], const CrtEnvironment *env) {
  if (!out || !tint || !env) return CRT_ERR_BAD_ARG;
  std::memset(out, 0, sizeof(*out));
  out->kind = CRT_LIGHT_DOME_MAP;
  out->geom_id = CRT_INVALID_ID;
  for (int i = 0; i < 3; i++) out->radiance[i] = tint[i];
  std::memcpy(&out->center[0], &env->p->id, 4);
  return CRT_OK;
}

}  // extern "C"
