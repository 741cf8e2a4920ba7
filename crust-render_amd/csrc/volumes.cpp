// The volume aggregate on the host: VolumeRegion::new (volume.rs:195-231) restated operation for operation, the image
// the seam kernels read (kernels/volume.hip.h: a 256-byte header, the region records, the grid data on a 256-byte
// boundary) and the handle's life. Building touches no device: the image is uploaded on first device use.
//
// Departures from the reference, all named in DESIGN.md §2: at most CRT_VOLUME_MAX_REGIONS regions and
// CRT_VOLUME_MAX_OCTAVES octaves; the placement is a 3x4 affine and world_to_local comes from affine_inverse (scene.cpp),
// not from glam's Mat4::inverse; a placement without a finite inverse and a non-finite field of a record are refused.
// A region whose majorant is <= 0 is accepted and skipped by the walk, as upstream (volume.rs:388-390).
#include <cstring>
#include <new>

#include "crt_internal.h"
#include "kernels/volume.hip.h"

namespace crt {

using dev::kVolMagic;
using dev::VolHeader;
using dev::VolRegionRec;

static inline float rust_max(float a, float b) { return (a > b || b != b) ? a : b; }  // f32::max
static inline float rust_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

static bool finite_all(const float *p, int n) {
  for (int i = 0; i < n; i++)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// CRT_OK and the image, or CRT_ERR_BAD_ARG with the reason in crt_last_error. Plain host C++: the stand-alone sanitizer
// program (profiles/host_shade/volume_sanitize.cpp) compiles this function without the rest of the library.
int volumes_build_image(const CrtVolumeRegion *regions, size_t n, const float *grid, size_t grid_len, std::vector<unsigned char> &image) {
  if (n > CRT_VOLUME_MAX_REGIONS) {
    set_error_text("crt_volumes_new: %zu regions (an aggregate holds at most %u)", n, CRT_VOLUME_MAX_REGIONS);
    return CRT_ERR_BAD_ARG;
  }
  if (n && !regions) { set_error_text("crt_volumes_new: no region records"); return CRT_ERR_BAD_ARG; }
  if (grid_len && !grid) { set_error_text("crt_volumes_new: %zu grid floats without an array", grid_len); return CRT_ERR_BAD_ARG; }
  if (grid_len > 0x3fffffffull) { set_error_text("crt_volumes_new: %zu grid floats (the image's offsets are 32-bit)", grid_len); return CRT_ERR_BAD_ARG; }
  VolRegionRec recs[CRT_VOLUME_MAX_REGIONS];
  std::memset(recs, 0, sizeof(recs));
  for (size_t i = 0; i < n; i++) {
    const CrtVolumeRegion &in = regions[i];
    VolRegionRec &R = recs[i];
    const bool finite = finite_all(in.local_to_world, 12) && finite_all(in.half_extent, 3) && finite_all(in.sigma_s, 3) &&
                        finite_all(in.sigma_a, 3) && finite_all(&in.g, 1) && finite_all(in.emission, 3) &&
                        finite_all(&in.density_scale, 1) && finite_all(&in.noise_scale, 1) && finite_all(&in.noise_gain, 3);
    if (!finite) { set_error_text("crt_volumes_new: region %zu has a field that is not finite", i); return CRT_ERR_BAD_ARG; }
    if (in.field > CRT_VOLUME_GRID) { set_error_text("crt_volumes_new: region %zu has the unknown field kind %u", i, in.field); return CRT_ERR_BAD_ARG; }
    if (in.field == CRT_VOLUME_NOISE && in.noise_octaves > CRT_VOLUME_MAX_OCTAVES) {
      set_error_text("crt_volumes_new: region %zu asks for %u noise octaves (at most %u)", i, in.noise_octaves, CRT_VOLUME_MAX_OCTAVES);
      return CRT_ERR_BAD_ARG;
    }
    float field_max = 1.0f;  // DensityField::max_value (volume.rs:74-83)
    if (in.field == CRT_VOLUME_GRID) {
      const uint64_t cells = (uint64_t)in.grid_dims[0] * in.grid_dims[1];
      const bool fits = cells <= 0xffffffffull && cells * in.grid_dims[2] <= 0xffffffffull;
      const uint64_t total = fits ? cells * in.grid_dims[2] : 0;
      if (!fits || total == 0 || total != in.grid_count) {
        set_error_text("crt_volumes_new: region %zu has a %u x %u x %u grid over %u values", i, in.grid_dims[0], in.grid_dims[1],
                       in.grid_dims[2], in.grid_count);
        return CRT_ERR_BAD_ARG;
      }
      if ((uint64_t)in.grid_offset + in.grid_count > grid_len) {
        set_error_text("crt_volumes_new: region %zu reads grid values %u .. %llu of %zu", i, in.grid_offset,
                       (unsigned long long)in.grid_offset + in.grid_count, grid_len);
        return CRT_ERR_BAD_ARG;
      }
      field_max = 0.0f;
      for (uint32_t k = 0; k < in.grid_count; k++) field_max = rust_max(field_max, grid[in.grid_offset + k]);
      R.nx = in.grid_dims[0]; R.ny = in.grid_dims[1]; R.nz = in.grid_dims[2];
      R.grid_off = in.grid_offset;
    }
    const float *m = in.local_to_world;
    const Affine l2w{f3(m[0], m[1], m[2]), f3(m[3], m[4], m[5]), f3(m[6], m[7], m[8]), f3(m[9], m[10], m[11])};
    const Affine w2l = affine_inverse(l2w);
    const float inv[12] = {w2l.x.x, w2l.x.y, w2l.x.z, w2l.y.x, w2l.y.y, w2l.y.z, w2l.z.x, w2l.z.y, w2l.z.z, w2l.t.x, w2l.t.y, w2l.t.z};
    if (!finite_all(inv, 12)) { set_error_text("crt_volumes_new: the placement of region %zu has no finite inverse", i); return CRT_ERR_BAD_ARG; }
    std::memcpy(R.w2l, inv, sizeof(inv));
    const F3 half = f3(in.half_extent[0], in.half_extent[1], in.half_extent[2]);
    const F3 ss = f3(in.sigma_s[0], in.sigma_s[1], in.sigma_s[2]) * in.density_scale;
    const F3 sa = f3(in.sigma_a[0], in.sigma_a[1], in.sigma_a[2]) * in.density_scale;
    const float inf = __builtin_inff();
    F3 mn = f3(inf, inf, inf), mx = f3(-inf, -inf, -inf);
    for (int c = 0; c < 8; c++) {
      const F3 corner = f3((c & 1) == 0 ? -half.x : half.x, (c & 2) == 0 ? -half.y : half.y, (c & 4) == 0 ? -half.z : half.z);
      const F3 w = affine_point(l2w, corner);
      mn = vmin(mn, w);
      mx = vmax(mx, w);
    }
    const F3 st = sa + ss;
    R.majorant = sse_max(sse_max(st.x, st.y), st.z) * field_max;
    R.field = in.field;
    R.g = rust_clamp(in.g, -0.99f, 0.99f);
    for (int a = 0; a < 3; a++) {
      R.half[a] = half[a]; R.bmin[a] = mn[a]; R.bmax[a] = mx[a];
      R.sigma_s[a] = ss[a]; R.sigma_a[a] = sa[a]; R.emission[a] = in.emission[a];
    }
    R.noise_scale = in.noise_scale; R.noise_octaves = in.noise_octaves; R.noise_gain = in.noise_gain;
    R.noise_lacunarity = in.noise_lacunarity; R.noise_threshold = in.noise_threshold; R.noise_seed = in.noise_seed;
  }
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  VolHeader hd;
  std::memset(&hd, 0, sizeof(hd));
  hd.magic = kVolMagic;
  hd.n_regions = (uint32_t)n;
  hd.region_bytes = (uint32_t)sizeof(VolRegionRec);
  hd.off_regions = (uint32_t)sizeof(VolHeader);
  hd.off_grid = (uint32_t)up(sizeof(VolHeader) + CRT_VOLUME_MAX_REGIONS * sizeof(VolRegionRec));
  hd.grid_floats = (uint32_t)grid_len;
  hd.bytes = (uint32_t)up(hd.off_grid + grid_len * 4 + 4);  // never empty: the kernels are handed a grid pointer
  image.assign(hd.bytes, 0);
  std::memcpy(image.data(), &hd, sizeof(hd));
  std::memcpy(image.data() + hd.off_regions, recs, sizeof(recs));
  if (grid_len) std::memcpy(image.data() + hd.off_grid, grid, grid_len * 4);
  return CRT_OK;
}

}  // namespace crt

#ifndef CRT_VOLUMES_BUILDER_ONLY

namespace crt {

struct Volumes {
  std::vector<unsigned char> image;
  uint32_t n_regions = 0;
  std::mutex mu;
  void *d_image = nullptr;  // uploaded on first device use
  ~Volumes() {
    if (d_image) {
      (void)hipDeviceSynchronize();  // nothing that was handed the image may still be reading it
      (void)hipFree(d_image);
    }
  }
};

}  // namespace crt

struct CrtVolumes { std::shared_ptr<crt::Volumes> p; std::atomic<int> refs{1}; };

namespace crt {

int volumes_device(CrtVolumes *v, VolumesView &out) {
  Volumes &V = *v->p;
  std::lock_guard<std::mutex> lock(V.mu);
  if (!V.d_image) {
    if (!device_ok()) return CRT_ERR_NO_DEVICE;
    void *d = nullptr;
    if (!CRT_HIP_OK(hipMalloc(&d, V.image.size()))) return CRT_ERR_NO_DEVICE;
    if (!CRT_HIP_OK(hipMemcpy(d, V.image.data(), V.image.size(), hipMemcpyHostToDevice))) { (void)hipFree(d); return CRT_ERR_NO_DEVICE; }
    V.d_image = d;
  }
  const VolHeader *hd = reinterpret_cast<const VolHeader *>(V.image.data());
  out.regions = reinterpret_cast<const VolRegionRec *>(static_cast<const unsigned char *>(V.d_image) + hd->off_regions);
  out.grid = reinterpret_cast<const float *>(static_cast<const unsigned char *>(V.d_image) + hd->off_grid);
  out.n_regions = hd->n_regions;
  return CRT_OK;
}

uint32_t volumes_region_count(const CrtVolumes *v) { return v->p->n_regions; }

void volumes_retain(CrtVolumes *v) { if (v) v->refs.fetch_add(1, std::memory_order_relaxed); }
void volumes_release(CrtVolumes *v) { if (v && v->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete v; }

}  // namespace crt

using namespace crt;

extern "C" {

CrtVolumes *crt_volumes_new(const CrtVolumeRegion *regions, size_t n, const float *grid, size_t grid_len) {
  CrtVolumes *out = nullptr;
  (void)abi_guard("crt_volumes_new", [&] {
    auto v = std::make_shared<Volumes>();
    const int rc = volumes_build_image(regions, n, grid, grid_len, v->image);
    if (rc != CRT_OK) return rc;
    v->n_regions = (uint32_t)n;
    CrtVolumes *handle = new CrtVolumes();
    handle->p = std::move(v);
    out = handle;
    return (int)CRT_OK;
  });
  return out;
}

void crt_volumes_free(CrtVolumes *v) { volumes_release(v); }

int crt_volumes_image(const CrtVolumes *v, const void **image, size_t *bytes) {
  if (!v || !image || !bytes) return CRT_ERR_BAD_ARG;
  *image = v->p->image.data();
  *bytes = v->p->image.size();
  return CRT_OK;
}

}  // extern "C"

#endif  // CRT_VOLUMES_BUILDER_ONLY
