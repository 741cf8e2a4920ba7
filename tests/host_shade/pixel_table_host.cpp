// The per-pixel camera table and the sample cursor (kernels/camera_pixel.hip.h) compiled as host C++ for
// tests/test_pixel_table_host.py, behind the stand-in <hip/hip_runtime.h> of profiles/host_shade. The truth is stated
// twice: camera_sample's computed form, restated here call for call from the sampler's functions (qmc.hip.h) as
// pathtrace.hip's camera_sample makes them, and the oracle's own statement of the sampler (oracle/ora_qmc.h).
//
// With -DPIXEL_TABLE_MAIN the file is a stand-alone program (its own pixel lists, the same checks) for a sanitizer build.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "camera_pixel.hip.h"
#include "ora_qmc.h"

using namespace crt::dev;

extern "C" {
// The table as the renderer's fill kernel writes it: eight words per owned pixel.
void pixel_table_fill(const uint32_t *pixels, size_t n, uint32_t width, int frame, uint32_t *out8) {
  for (size_t i = 0; i < n; i++) {
    const PixelRec r = pixel_record(pixels[i], width, frame);
    std::memcpy(out8 + 8 * i, &r, 32);
  }
}
// The same eight words as camera_sample's computed form works them out for one sample of the pixel (the sample index
// rides along in the Sampler and reaches none of them), and as the oracle's sampler does.
void pixel_table_computed(const uint32_t *pixels, size_t n, uint32_t width, int frame, int index, uint32_t *out8, uint32_t *ora8) {
  for (size_t i = 0; i < n; i++) {
    const uint32_t lin = pixels[i];
    const uint32_t px = lin % width, py = lin / width;
    const int tile = (int)(px >> 8) + (int)(py >> 8) * 4096;
    {
      const Sampler root = new_domain(sampler_new((int)px, (int)py, frame, index), tile);
      const Sampler cam = new_domain(root, 0 /* K_CAMERA */);
      uint32_t *o = out8 + 8 * i;
      o[0] = __float_as_uint((float)px); o[1] = __float_as_uint((float)py);
      o[2] = pcg_hash(cam.pattern);
      for (uint32_t d = 0; d < 4; d++) o[3 + d] = pcg_hash(cam.pattern + d + 1u);
      o[7] = new_domain(root, 1 /* K_PATH */).pattern;
    }
    {
      const OraSampler root = ora_new_domain(ora_sampler_new((int)px, (int)py, frame, index), tile);
      const OraSampler cam = ora_new_domain(root, 0);
      uint32_t *o = ora8 + 8 * i;
      o[0] = __float_as_uint((float)px); o[1] = __float_as_uint((float)py);
      o[2] = ora_pcg_hash(cam.pattern);
      for (uint32_t d = 0; d < 4; d++) o[3 + d] = ora_pcg_hash(cam.pattern + d + 1u);
      o[7] = ora_new_domain(root, 1).pattern;
    }
  }
}
// Draws off the table's seeds against draw_sample4 on the K_CAMERA domain and the oracle's draw, for `n_idx` sample
// indices per pixel: the number of (pixel, index) pairs whose four floats differ in any bit from either.
size_t pixel_table_draw_mismatches(const uint32_t *pixels, size_t n, uint32_t width, int frame, const uint32_t *indices, size_t n_idx) {
  static uint32_t tab[kSobolLdsWords];
  sobol_tables_init(tab);
  size_t bad = 0;
  for (size_t i = 0; i < n; i++) {
    const PixelRec r = pixel_record(pixels[i], width, frame);
    const uint32_t px = pixels[i] % width, py = pixels[i] / width;
    const int tile = (int)(px >> 8) + (int)(py >> 8) * 4096;
    for (size_t k = 0; k < n_idx; k++) {
      float a[4], b[4], c[4];
      draw_sample4_seeded(indices[k], r.seed, a, tab);
      draw_sample4(new_domain(new_domain(sampler_new((int)px, (int)py, frame, (int)indices[k]), tile), 0), b, tab);
      ora_draw_sample4(ora_new_domain(ora_new_domain(ora_sampler_new((int)px, (int)py, frame, (int)indices[k]), tile), 0), c);
      if (std::memcmp(a, b, 16) != 0 || std::memcmp(a, c, 16) != 0) bad++;
    }
  }
  return bad;
}
// A lane's cursor from g0 over `rounds` rounds of `step`: the rounds at which (pix, sl) differ from (g % n_act, g / n_act).
size_t sample_cursor_mismatches(unsigned long long g0, unsigned long long step, uint32_t n_act, uint32_t rounds) {
  SampleCursor c = sample_cursor(g0, step, n_act);
  size_t bad = 0;
  unsigned long long g = g0;
  for (uint32_t r = 0; r < rounds; r++, g += step) {
    if (c.pix != (uint32_t)(g % n_act) || c.sl != (uint32_t)(g / n_act)) bad++;
    sample_cursor_next(c, n_act);
  }
  return bad;
}
}

#ifdef PIXEL_TABLE_MAIN
// 16x16 tiles dealt round-robin over the ranks, row-major inside a tile: a shard's pixel list as the renderer holds it.
static std::vector<uint32_t> shard(uint32_t w, uint32_t h, uint32_t rank, uint32_t world) {
  std::vector<uint32_t> out;
  uint32_t t = 0;
  for (uint32_t ty = 0; ty < h; ty += 16)
    for (uint32_t tx = 0; tx < w; tx += 16, t++) {
      if (t % world != rank) continue;
      for (uint32_t y = ty; y < ty + 16 && y < h; y++)
        for (uint32_t x = tx; x < tx + 16 && x < w; x++) out.push_back(y * w + x);
    }
  return out;
}
int main() {
  size_t bad = 0;
  const uint32_t w = 64, h = 32;
  const uint32_t idx[] = {0u, 1u, 2u, 7u, 255u, 256u, 511u, 65535u, 0x12345678u};
  for (uint32_t rank : {0u, 2u}) {  // 3 and 2 of the frame's 8 tiles
    const std::vector<uint32_t> pix = shard(w, h, rank, 3);
    std::vector<uint32_t> a(8 * pix.size()), b(a.size()), c(a.size());
    for (int frame : {0, 7}) {
      pixel_table_fill(pix.data(), pix.size(), w, frame, a.data());
      pixel_table_computed(pix.data(), pix.size(), w, frame, 5, b.data(), c.data());
      for (size_t k = 0; k < a.size(); k++) bad += (a[k] != b[k]) + (a[k] != c[k]);
      bad += pixel_table_draw_mismatches(pix.data(), pix.size(), w, frame, idx, sizeof idx / sizeof idx[0]);
    }
  }
  for (uint32_t n_act : {1u, 255u, 256u, 257u, 20736u})
    for (uint32_t grid : {1u, 3u, 2048u})
      for (uint32_t lane : {0u, 255u})
        bad += sample_cursor_mismatches((unsigned long long)(grid - 1) * 256 + lane, (unsigned long long)grid * 256, n_act, 40);
  bad += sample_cursor_mismatches((1ull << 32) + 12345ull, 2048ull * 256, 4000000000u, 40);
  bad += sample_cursor_mismatches((1ull << 40) + 99ull, 16384ull * 256, 2073600u, 40);
  std::printf("pixel table and sample cursor: %zu mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
