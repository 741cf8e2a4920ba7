// What a camera sample owes to its PIXEL alone (pathtrace.hip, camera_sample): the pixel's coordinates, the K_CAMERA
// domain's five Owen seeds and the K_PATH domain's pattern depend on the owned-pixel slot and the frame number, both fixed
// when a renderer is created — yet the sample loop worked them out for every one of a pixel's samples: ten pcg_hash, a
// 32-bit division with remainder and two int-to-float conversions. A renderer derives them once per owned pixel
// (k_fill_pixel_table -> pixel_record below) through the sampler's own functions (qmc.hip.h: sampler_new, new_domain,
// owen_seeds), so every stored word has the bits the loop would have computed, and the camera launches load the 32-byte
// record instead (CRT_PIXEL_TABLE=0: never).
//
// Also here: the sample cursor. A lane's global sample number advances by one grid's width per round of the camera
// launch; its pixel slot g % n_act and sample g / n_act — a 64-bit division each per sample — follow from the previous
// round's by one add and one conditional wrap.
//
// Plain inline functions over qmc.hip.h: compiled for the device by pathtrace.hip and for the host by the tests.
#pragma once

#include "qmc.hip.h"

namespace crt {
namespace dev {

constexpr int kDomainCamera = 0, kDomainPath = 1;  // tracer.rs:20-22: the K_CAMERA and K_PATH keys off the root domain

// One owned pixel's record, 32 bytes = two 16-byte loads. px and py are stored as the floats the sample loop converts
// them to ((float)px is exact below 2^24; a wider frame builds no table).
struct PixelRec {
  float px, py;          // (float)(lin % width), (float)(lin / width)
  uint32_t seed[5];      // owen_seeds of the K_CAMERA domain's pattern: the index scramble, then dimensions 0..3
  uint32_t path_pattern; // new_domain(root, K_PATH).pattern
};
static_assert(sizeof(PixelRec) == 32, "two 16-byte loads per camera sample");

// The root domain of a pixel's sampler (tracer.rs:543, :559-561): PathSampler::new(px, py, frame, index).new_domain(tile).
__device__ __forceinline__ Sampler pixel_root(uint32_t px, uint32_t py, int frame, int index) {
  const int tile = (int)(px >> 8) + (int)(py >> 8) * 4096;  // tracer.rs:543
  return new_domain(sampler_new((int)px, (int)py, frame, index), tile);
}
__device__ __forceinline__ PixelRec pixel_record(uint32_t lin, uint32_t width, int frame) {
  const uint32_t px = lin % width, py = lin / width;
  const Sampler root = pixel_root(px, py, frame, 0);  // the index rides along: no pattern depends on it
  PixelRec r;
  r.px = (float)px; r.py = (float)py;
  owen_seeds(new_domain(root, kDomainCamera).pattern, r.seed);
  r.path_pattern = new_domain(root, kDomainPath).pattern;
  return r;
}

// Pixel slot and sample of a lane's global sample number g as g advances by `step` per round: pix = g % n_act,
// sl = g / n_act. n_act > 0; g and step are any 64-bit values whose quotients fit 32 bits (the staging film's slots do).
struct SampleCursor { uint32_t pix, sl, step_pix, step_sl; };
__device__ __forceinline__ SampleCursor sample_cursor(unsigned long long g, unsigned long long step, uint32_t n_act) {
  SampleCursor c;
  c.pix = (uint32_t)(g % n_act); c.sl = (uint32_t)(g / n_act);
  c.step_pix = (uint32_t)(step % n_act); c.step_sl = (uint32_t)(step / n_act);
  return c;
}
__device__ __forceinline__ void sample_cursor_next(SampleCursor &c, uint32_t n_act) {
  const uint32_t room = n_act - c.step_pix;  // 1..n_act; no sum of two slots is formed: n_act may be close to 2^32
  const bool wrap = c.pix >= room;
  c.pix = wrap ? c.pix - room : c.pix + c.step_pix;
  c.sl += c.step_sl + (wrap ? 1u : 0u);
}

}  // namespace dev
}  // namespace crt
