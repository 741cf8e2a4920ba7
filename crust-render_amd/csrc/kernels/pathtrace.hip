// Wavefront path tracer for gfx950: crust-core's integrator (surface arm + carried interior media) as data-parallel
// stages over device-resident queues.
//
// What it computes: crates/crust-core/src/tracer.rs:515-636 (render_pixel), :1086-1558 (trace_path: surface arm,
// :1159-1165 / :1256-1319 / :1352-1360 carried medium), :930-953 (bounce_emission_weight), :1016-1035 (shadow
// test), :85-104 (MIS weights), :1478-1490 (Russian roulette), :1327-1340 (sky), rt_world.rs:207-237,
// light.rs:421-440 — with the backward gather (tracer.rs:1537-1557) restated as the algebraically identical forward
// accumulation
//     L += beta * (atten * emitted) * w     (bounce-hit emission, weighted for the previous vertex)
//     L += (beta * atten) * emit_here       (primary vertex / after a medium scatter)
//     L += (beta * atten) * nee             (after the shadow ray)
//     beta *= atten * value * cos / pdf     (then / p_survive under roulette)
// in exactly that order, which is the order the CPU oracle's forward mode uses, so the two agree bit for bit.
//
// Stages (device functions; k_path runs them all for a workgroup-private queue segment in one launch, the k_*
// kernels one at a time — no host sync either way):
//   generate : camera samples -> path state (SoA), one slot per (pixel, sample), dealt to the segments round-robin
//   extend   : closest-hit traversal of the segment's live paths            -> hit records
//   shade    : medium free flight, emission + MIS, light sampling -> shadow queue, BSDF sampling, roulette;
//              survivors are compacted into the other state buffer of the SAME segment with a wave ballot +
//              popcount prefix and an LDS counter (no global atomics); finished paths write their radiance to the
//              film staging plane
//   shadow   : any-hit traversal of the segment's shadow queue; unoccluded requests add their contribution
//   resolve  : staging planes are folded into the film in sample order (sum += color, tracer.rs:599)
// Path state is struct-of-arrays of 16-byte records, so every stage's loads and stores are unit-stride across a wave.
//
// This file is the device side only: the kernels, then the instance table and what the host needs from it
// (resolve_kernels, kStageKernels, kKernelBuild — declared in ../render_kernels.h with the launch argument types). The
// renderer that launches them — buffers, lanes, the bounce loop, the C ABI — is ../render.cpp.
#include <cstddef>

#define CRT_GUIDING_BOUNCE  // guiding.hip.h (first included by render_kernels.h) with the guided bounce: k_shade_guided
#include "../render_kernels.h"
#include "camera_pixel.hip.h"
#include "shade.hip.h"
#include "faces.hip.h"
#include "guiding.hip.h"
#include "traverse_camera.hip.h"
#include "traverse_pool.hip.h"
#include "vertex_simple.hip.h"
#include "volume.hip.h"

namespace crt {

using namespace dev;

namespace {

// Occupancy targets (second __launch_bounds__ argument = waves per SIMD; caps the VGPR allocation).
#ifndef CRT_EXTEND_WAVES
#define CRT_EXTEND_WAVES 3
#endif
#ifndef CRT_SHADE_WAVES
#define CRT_SHADE_WAVES 3
#endif
#ifndef CRT_SHADOW_WAVES
#define CRT_SHADOW_WAVES 3
#endif

enum { K_CAMERA = 0, K_PATH = 1, K_TIME = 2 };                 // tracer.rs:20-22 (off root)
static_assert(K_CAMERA == kDomainCamera && K_PATH == kDomainPath, "camera_pixel.hip.h derives the same domains");
// (the domains off a vertex, K_NEE .. K_VOLUME, and the roulette constants: vertex_simple.hip.h)
constexpr uint32_t kFilmTarget = 0x80000000u;
constexpr uint32_t kPrevValid = 1u << 16, kPrevDelta = 1u << 17;
constexpr int kMediumShift = 18;             // aux[18:32): 1-based compact id of the interior medium the ray travels in (at most kMaxMedia)
// Volume renders (k_volume): a path that scattered inside a region carries one of these four words where its hit record's
// geometry word was — bit 0: the path survived its roulette, bit 1: the phase vertex asks for a shadow ray. No geometry id
// reaches them (a material table has fewer than 2^31 - 16 records), and kInvalid (a miss) is none of them.
constexpr uint32_t kVolScatter = 0xfffffff0u;
__device__ __forceinline__ bool vol_scatter_word(uint32_t hg) { return hg >= kVolScatter && hg < kVolScatter + 4u; }

// Streaming accesses (path state, hit records, queues, staging film: written once, read once a whole segment pass
// later — far beyond any cache) carry the non-temporal hint, so they do not push the BVH's nodes, instance records
// and instance records out of L2: +0.8 % (veach_mis) to +2.6 % (PointInstancedMedCity 3840x2160) over plain accesses
// (profiles/README.md, r02h). CRT_NT=0 builds plain accesses (A/B).
#ifndef CRT_NT
#define CRT_NT 1
#endif
typedef float nt_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t nt_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st_nt(float4 *p, float4 v) {
  if (CRT_NT) { nt_f4 x = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(x, reinterpret_cast<nt_f4 *>(p)); }
  else *p = v;
}
__device__ __forceinline__ void st_nt(uint4 *p, uint4 v) {
  if (CRT_NT) { nt_u4 x = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(x, reinterpret_cast<nt_u4 *>(p)); }
  else *p = v;
}
__device__ __forceinline__ void st_nt(uint32_t *p, uint32_t v) {
  if (CRT_NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}
__device__ __forceinline__ void st_nt(float *p, float v) {
  if (CRT_NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}
// Hit records are the one stream written OUT OF ORDER (a ray's record goes out when its traversal ends): 16 + 4 bytes
// into two planes, each a partial 32-byte sector. CRT_NT_HIT=0 writes them as plain stores, which L2 may merge with the
// neighbouring slots' before they leave for HBM (A/B: profiles/README.md, round 3).
#ifndef CRT_NT_HIT
#define CRT_NT_HIT CRT_NT
#endif
__device__ __forceinline__ void st_hit(float4 *p, float4 v) { if (CRT_NT_HIT) st_nt(p, v); else *p = v; }
__device__ __forceinline__ void st_hit(uint32_t *p, uint32_t v) { if (CRT_NT_HIT) st_nt(p, v); else *p = v; }
__device__ __forceinline__ float4 ld_nt(const float4 *p) {
  if (CRT_NT) { const nt_f4 x = __builtin_nontemporal_load(reinterpret_cast<const nt_f4 *>(p)); return make_float4(x.x, x.y, x.z, x.w); }
  return *p;
}



__device__ __forceinline__ uint32_t dir_bin(float dx, float dy, float dz) {
  if (kBins == 1) return 0;
  return (dx < 0.0f ? 1u : 0u) | (dy < 0.0f ? 2u : 0u) | (dz < 0.0f ? 4u : 0u);
}
// Prefix sums of a workgroup's kBins sub-segment counts (pre[kBins] = total); ends with a barrier.
// The counts are read as volatile: in the fused kernel they were written earlier in the same launch by another wave
// of this workgroup, so the read must be a fresh vector load, never a scalar-cache or hoisted one.
__device__ __forceinline__ void bins_prefix(const uint32_t *counts, uint32_t *pre /* LDS, kBins + 1 */) {
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (int b = 0; b < kBins; b++) { pre[b] = acc; acc += ((const volatile uint32_t *)counts)[b]; }
    pre[kBins] = acc;
  }
  __syncthreads();
}
// Slot of the k-th live path of this workgroup (sub-segments concatenated in bin order).
__device__ __forceinline__ uint32_t bin_slot(uint32_t k, const uint32_t *pre, uint32_t seg_cap) {
  uint32_t b = 0;
#pragma unroll
  for (int t = 1; t < kBins; t++) b += k >= pre[t] ? 1u : 0u;
  return (blockIdx.x * kBins + b) * seg_cap + (k - pre[b]);
}


__device__ __forceinline__ float light_weight(int s, float light_pdf, float bounce_pdf) {  // tracer.rs:85-92
  switch (s) {
    case CRT_STRATEGY_POWER: return power_heuristic(light_pdf, bounce_pdf);
    case CRT_STRATEGY_BALANCE: return balance_heuristic(light_pdf, bounce_pdf);
    case CRT_STRATEGY_LIGHT: return 1.0f;
    default: return 0.0f;
  }
}
__device__ __forceinline__ float bounce_weight(int s, float bounce_pdf, float light_pdf) {  // tracer.rs:97-104
  switch (s) {
    case CRT_STRATEGY_POWER: return power_heuristic(bounce_pdf, light_pdf);
    case CRT_STRATEGY_BALANCE: return balance_heuristic(bounce_pdf, light_pdf);
    case CRT_STRATEGY_LIGHT: return 0.0f;
    default: return 1.0f;
  }
}
// What an escaping ray picks up (tracer.rs:1321-1342 with escaped_emission, :966-1009): every light at infinity
// covering the direction, MIS-weighted against the previous vertex's NEE; the sky gradient only where none covers.
__device__ __forceinline__ V3 sky_gradient(V3 unit_direction) {
  const float t = 0.5f * (unit_direction.y + 1.0f);
  return v3(1.0f, 1.0f, 1.0f) * (1.0f - t) + v3(0.5f, 0.7f, 1.0f) * t;
}
// A path that leaves a scene without lights at infinity ends on the sky gradient (tracer.rs:1321-1342): the one expression
// of the miss steps of shade and of generate's root cull, so the three write the same bits.
__device__ __forceinline__ V3 escaped_to_sky(V3 rd, V3 beta, V3 L) {
  const V3 unit_direction = normalize(rd);
  const V3 background = splat(0.0f) + sky_gradient(unit_direction);
  return L + beta * background;
}
template <bool ENV = false>
__device__ __forceinline__ V3 escaped_background(const CrtLight *lights, uint32_t n_lights, int strategy,
                                                 V3 unit_direction, bool competing, float prev_pdf, const EnvSlot *envs = nullptr) {
  V3 background = splat(0.0f);
  bool covered = false;
  for (uint32_t k = 0; k < n_lights; k++) {
    V3 emitted;
    float pdf;
    if (!light_escaped_env<ENV>(lights[k], envs, unit_direction, emitted, pdf)) continue;
    covered = true;
    float weight = 1.0f;
    if (competing && strategy != CRT_STRATEGY_BSDF) {
      const float light_pdf = rmax(pdf / (float)n_lights, 1e-6f);
      weight = bounce_weight(strategy, prev_pdf, light_pdf);
    }
    background = background + emitted * weight;
  }
  if (!covered) background = background + sky_gradient(unit_direction);
  return background;
}

__device__ __forceinline__ bool lds_take(bool want, uint32_t *next, uint32_t limit, uint32_t &idx) {
  const unsigned long long mask = __ballot(want);
  if (mask == 0) return false;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mask) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(next, (uint32_t)__popcll(mask));
  base = __shfl(base, leader, 64);
  idx = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
  return want && idx < limit;
}

// Segment-local append: every lane with `want` gets a unique slot of its workgroup's segment. The wave's
// lanes are ranked with a ballot + popcount prefix; one LDS atomic per wave reserves the run.
__device__ __forceinline__ uint32_t seg_append(bool want, uint32_t *lds_counter) {
  const unsigned long long mask = __ballot(want);
  if (mask == 0) return 0;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mask) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(lds_counter, (uint32_t)__popcll(mask));
  base = __shfl(base, leader, 64);
  return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// Per-workgroup reduction of a statistics counter: LDS first, then one global atomic per workgroup.
__device__ __forceinline__ void add_stat(uint32_t *lds_slot, uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(lds_slot, v);
}

// ---- interior media of the materials (openpbr.rs:225-258), derived once on the device so that the logarithms
// are the same deterministic sequence the shading kernels use. Two launches: every record in parallel (40 008 of them on
// the instanced city: one thread looping took 31.6 ms), then ONE workgroup numbers the present ones in material order —
// each thread counts a contiguous run of the table, an LDS prefix over the 1024 runs, ids handed out run by run. ----
__global__ void k_build_media(const CrtMaterial *materials, uint32_t n, DevMedium *media) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  DevMedium m;
  medium_from_material(materials[i], m);
  m.id = 0;
  media[i] = m;
}
// ---- the per-material constants of the vertex code (shade.hip.h, DevMaterial), derived once per renderer with the
// inline functions the vertex code itself runs on a raw record: the same operations, so the same bits. ----
__global__ void k_derive_materials(const CrtMaterial *materials, uint32_t n, DevMaterial *derived) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  DevMaterial d;
  derive_material(materials[i], d);
  derived[i] = d;
}
// The table a shade instance stages and indexes, and its view of record i.
template <bool DRV> struct MatTable;
template <> struct MatTable<false> {
  typedef CrtMaterial Rec;
  __device__ __forceinline__ static const Rec *of(const Params &P) { return P.materials; }
  __device__ __forceinline__ static MatRaw view(const Rec *table, const Params &, uint32_t i) { return MatRaw{table[i]}; }
};
template <> struct MatTable<true> {
  typedef DevMaterial Rec;
  __device__ __forceinline__ static const Rec *of(const Params &P) { return P.mat_derived; }
  __device__ __forceinline__ static MatDerived view(const Rec *table, const Params &P, uint32_t i) { return MatDerived{table[i], P.materials[i]}; }
};
__global__ __launch_bounds__(kNumberBlock) void k_number_media(uint32_t n, DevMedium *media, DevMedium *by_id, uint32_t *count_out) {
  __shared__ uint32_t run_sum[kNumberBlock];
  const uint32_t per = (n + kNumberBlock - 1) / kNumberBlock;
  const uint32_t lo = threadIdx.x * per < n ? threadIdx.x * per : n, hi = lo + per < n ? lo + per : n;
  uint32_t mine = 0;
  for (uint32_t i = lo; i < hi; i++) mine += media[i].present ? 1u : 0u;
  run_sum[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < kNumberBlock; off <<= 1) {  // inclusive Hillis-Steele prefix
    const uint32_t add = (int)threadIdx.x >= off ? run_sum[threadIdx.x - off] : 0u;
    __syncthreads();
    run_sum[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t count = run_sum[threadIdx.x] - mine;  // present records before this run
  for (uint32_t i = lo; i < hi; i++) {
    if (!media[i].present) continue;
    count++;
    if (count <= kMaxMedia) {
      media[i].id = count;
      by_id[count - 1] = media[i];
    }
  }
  if (threadIdx.x == kNumberBlock - 1) *count_out = run_sum[threadIdx.x];
}

// ---- generate: PathSampler::new(...).new_domain(tile), camera sample, camera ray (tracer.rs:559-585) ----
// Every stage body below is a device function working on the calling workgroup's own queue segment, with its big
// LDS buffer passed in: the per-stage kernels hand it their own array, the fused kernel (k_path) one shared arena.
constexpr int kArenaDwords = kEngineLdsDwords > kSobolLdsWords ? kEngineLdsDwords : kSobolLdsWords;
static_assert(sizeof(CrtMaterial) % 4 == 0, "material records are copied as dwords");
// Shade's pending rings (one per material class) sit at the END of the arena, the material table between the Sobol
// tables and the rings.
constexpr uint32_t kRing = 2 * kBlock;                 // entries per class ring: < kBlock pending + one classify batch
constexpr int kRingDwords = kClasses * (int)kRing;
constexpr int kClassLdsMax = 1024;                     // geom ids whose class byte is staged in LDS (1 KB)
// (The pipelined four-wave instance has a budget of its own — staging blocks instead of class rings: kPipeMatMax below.)
constexpr int mat_lds_max(int arena) { return (arena - kSobolLdsWords - kRingDwords - kClassLdsMax / 4) / (int)(sizeof(CrtMaterial) / 4); }
// The per-stage shade kernel of simple-material scenes without lights at infinity also runs four workgroups per CU
// (128 registers, a 40 KB arena: cornellbox +2 %); the other instances spill too much at 128 registers (sun_sky -16 %).
#ifndef CRT_SHADE_WIDE_WAVES
#define CRT_SHADE_WIDE_WAVES 4  // workgroups per CU of the WIDE shade kernel (5: 96 registers, a 31 KB arena — A/B, round 3)
#endif
constexpr int kArenaWide = (160 / CRT_SHADE_WIDE_WAVES) * 1024 / 4 - 256;
static_assert(mat_lds_max(kArenaWide) >= 16 && mat_lds_max(kArenaDwords) >= 16, "the arena holds the Sobol tables, the rings and a material table");

// (The material classes the rings are per: launch_plan.h, material_class.)

// One camera sample (tracer.rs:559-585): PathSampler::new(...).new_domain(tile), filter jitter, lens, primary ray, the
// K_PATH domain's pattern. g = the sample's global number within the batch: active pixel g % n_act, sample g / n_act.
struct CameraSample { V3 o, d; float time; uint32_t pattern, pix, sl; };
__device__ __forceinline__ CameraSample camera_sample(const Params &P, size_t g, uint32_t sample_begin, const uint32_t *sobol_tab) {
  CameraSample cs;
  cs.pix = (uint32_t)(g % P.n_act); cs.sl = (uint32_t)(g / P.n_act);  // pix: active slot
  const uint32_t lin = P.pixel_index[P.active ? P.active[cs.pix] : cs.pix];
  const uint32_t px = lin % P.width, py = lin / P.width;
  const int tile = (int)(px >> 8) + (int)(py >> 8) * 4096;  // tracer.rs:543
  const Sampler root = new_domain(sampler_new((int)px, (int)py, P.frame, (int)(sample_begin + cs.sl)), tile);
  float cam[4];
  draw_sample4(new_domain(root, K_CAMERA), cam, sobol_tab);
  const float fx = filter_offset(P.filter_kind, P.filter_radius, cam[0]);
  const float fy = filter_offset(P.filter_kind, P.filter_radius, cam[1]);
  const float u = ((float)px + fx) / (float)P.width;
  const float v = ((float)py + fy) / (float)P.height;
  cs.time = 0.0f;
  if (P.has_motion) {  // tracer.rs:579-583
    float t4[4];
    draw_sample4(new_domain(root, K_TIME), t4, sobol_tab);
    cs.time = t4[0];
  }
  camera_get_ray(P.camera, u, v, cam[2], cam[3], cs.o, cs.d);
  cs.pattern = new_domain(root, K_PATH).pattern;  // tracer.rs:1101
  return cs;
}
// Camera samples are dealt to the workgroup segments in round-robin chunks of one workgroup's width: slot k of
// segment b holds global sample g = ((k / 256) * G + b) * 256 + k % 256. Every segment is then a uniform
// sample of the frame (sky and geometry alike), so the per-segment work stays balanced at every bounce, while
// a wave still holds 64 consecutive pixels of one 16x16 tile (coherent primary rays).
__device__ __forceinline__ size_t camera_slot_sample(size_t k) {
  return ((k / kBlock) * (size_t)gridDim.x + blockIdx.x) * kBlock + (k % kBlock);
}

// camera_sample's second form (camera_pixel.hip.h): what depends on the pixel alone comes from the renderer's table, one
// record per owned-pixel slot, and (pix, sl) from the caller's sample cursor. The arithmetic left — the index scramble,
// the Sobol draw, the filter offsets, the ray — is the first form's on the same words, so the two return the same bits.
// Static pinhole batches only (the camera launches' plans): no K_TIME draw.
// The record's two 16-byte halves come from pixel_rec_load, which the camera launches issue a round ahead: a lane's next
// pixel slot is its cursor's (always below n_act, past the batch's end too), so the load flies behind the trace of the
// current ray instead of heading a round trip at the top of every round.
__device__ __forceinline__ void pixel_rec_load(const Params &P, const PixelRec *table, uint32_t pix, uint4 &r0, uint4 &r1) {
  const uint4 *rec = reinterpret_cast<const uint4 *>(table + (P.active ? P.active[pix] : pix));
  r0 = rec[0]; r1 = rec[1];
}
__device__ __forceinline__ CameraSample camera_sample_table(const Params &P, uint4 r0, uint4 r1, uint32_t pix, uint32_t sl,
                                                            uint32_t sample_begin, const uint32_t *sobol_tab) {
  CameraSample cs;
  cs.pix = pix; cs.sl = sl;
  const uint32_t seed[5] = {r0.z, r0.w, r1.x, r1.y, r1.z};
  float cam[4];
  draw_sample4_seeded(sample_begin + sl, seed, cam, sobol_tab);
  const float fx = filter_offset(P.filter_kind, P.filter_radius, cam[0]);
  const float fy = filter_offset(P.filter_kind, P.filter_radius, cam[1]);
  const float u = (__uint_as_float(r0.x) + fx) / (float)P.width;
  const float v = (__uint_as_float(r0.y) + fy) / (float)P.height;
  cs.time = 0.0f;
  camera_get_ray(P.camera, u, v, cam[2], cam[3], cs.o, cs.d);
  cs.pattern = r1.w;
  return cs;
}
// The root cull's predicate on the root as stage_nodes laid it out in the LDS window (seven 16-byte parts: three of
// lower bounds, three of upper bounds, the child words — WideNode's own order): node_touched on the same 28 words.
__device__ __forceinline__ bool root_touched_lds(const uint32_t *node, V3 o, V3 d) {
  const float4 *nb = reinterpret_cast<const float4 *>(node);
  float bmin[3][4], bmax[3][4];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float4 lo = nb[a], hi = nb[3 + a];
    bmin[a][0] = lo.x; bmin[a][1] = lo.y; bmin[a][2] = lo.z; bmin[a][3] = lo.w;
    bmax[a][0] = hi.x; bmax[a][1] = hi.y; bmax[a][2] = hi.z; bmax[a][3] = hi.w;
  }
  const uint4 ch = *reinterpret_cast<const uint4 *>(nb + 6);
  const uint32_t child[4] = {ch.x, ch.y, ch.z, ch.w};
  return node_touched(bmin, bmax, child, o.x, o.y, o.z, d.x, d.y, d.z, 0.001f, CRT_INF);
}
// One record per owned-pixel slot, once per renderer (crt_renderer_new): the frame number and the pixel list never change.
__global__ void k_fill_pixel_table(const uint32_t *pixel_index, uint32_t n_pix, uint32_t width, int frame, PixelRec *table) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pix) return;
  table[i] = pixel_record(pixel_index[i], width, frame);
}

// A compact camera path (Params::cam_compact) read back: direction and pattern from plane `a`, origin = the pinhole
// camera's (camera_get_ray with no lens offset: origin + 0), pixel and sample from the slot's sample number (< 2^31:
// ensure_buffers). D = plane d's words as generate would have written them — under the root cull (cam_compact == 2) the
// words generate DID write: the caller has read plane d into D, the slot of a compacted survivor says nothing. PLANE_D:
// the instance holds that form (the simple-material shade kernels; the general ones are at their register limit and
// run the full form under the root cull instead — plan_launches).
template <bool PLANE_D>
__device__ __forceinline__ void compact_camera_path(const Params &P, uint32_t k, float4 a, float4 &A, float4 &B, uint4 &D) {
  const V3 o = ld3(P.camera.origin) + splat(0.0f);
  A = make_float4(o.x, o.y, o.z, a.x);
  B = make_float4(a.y, a.z, 1.0f, 1.0f);
  if (PLANE_D && P.cam_compact == 2) return;  // uniform
  const uint32_t g = (uint32_t)camera_slot_sample(k);
  D = make_uint4(__float_as_uint(a.w), g % P.n_act, (P.max_depth & 0xffffu) << 16, g / P.n_act);
}

// Plane `c` of a camera path is a constant (throughput 1, radiance 0): the per-stage pipeline neither writes it here nor
// reads it in its first shade (17 GB per 531 M-path batch, +1.3 %; the fused kernel keeps the plain form — measured
// slower there with the special case). CRT_REGEN_FIRST=1 goes further — plane `d` (sampler pattern, pixel, depth, sample)
// is not written either and the first shade reads NOTHING of the path state: it works the camera sample out again from
// the slot number (Sobol tables in LDS). Measured on the bench (round 3, profiles/README.md): generate + resolve -1.2 ms
// per step, shade +3 ms — the first shade is bound by its dependent round trips and barriers, not by the 68-116 bytes
// per path this saves, and the ~350 more instructions per path are not free. Off.
#ifndef CRT_REGEN_FIRST
#define CRT_REGEN_FIRST 0
#endif
constexpr bool kRegenFirst = CRT_REGEN_FIRST != 0;
#ifndef CRT_CAM_COMPACT_BUILD
#define CRT_CAM_COMPACT_BUILD 1  // 0: the 16-byte camera path form is compiled out of generate, extend and shade (A/B)
#endif
#ifndef CRT_MAT_INDEX_BUILD
#define CRT_MAT_INDEX_BUILD 1    // 0: shade indexes the material table by geometry id only (A/B; the host then never deduplicates)
#endif
static_assert(kBins == 1 || !CRT_REGEN_FIRST, "the first shade takes a camera path's sample number from its slot: one sub-segment per workgroup");
__device__ __forceinline__ void generate_segment(const Params &P, const PathSoA &S, Counters *C, uint32_t sample_begin,
                                                 uint32_t n_samples, uint32_t *sobol_tab /* kSobolLdsWords */, bool write_c) {
  sobol_tables_init(sobol_tab);
  const size_t total = (size_t)P.n_act * n_samples;
  const size_t seg0 = (size_t)blockIdx.x * kBins * P.seg_cap;  // camera rays are coherent as dealt: all in bin 0
  uint32_t seg_n = 0;
  for (size_t k = threadIdx.x; k < P.seg_cap; k += kBlock) {
    const size_t g = camera_slot_sample(k);
    if (g >= total) break;
    seg_n = (uint32_t)k + 1;
    const size_t i = seg0 + k;
    const CameraSample cs = camera_sample(P, g, sample_begin, sobol_tab);
    if (CRT_CAM_COMPACT_BUILD && !write_c && P.cam_compact) {  // 16 of the 48-64 bytes: the rest is constant or follows from the slot
      st_nt(&S.a[i], make_float4(cs.d.x, cs.d.y, cs.d.z, __uint_as_float(cs.pattern)));
      continue;
    }
    st_nt(&S.a[i], make_float4(cs.o.x, cs.o.y, cs.o.z, cs.d.x));
    st_nt(&S.b[i], make_float4(cs.d.y, cs.d.z, 1.0f, 1.0f));
    if (write_c) st_nt(&S.c[i], make_float4(1.0f, 0.0f, 0.0f, 0.0f));
    if (write_c || !kRegenFirst) st_nt(&S.d[i], make_uint4(cs.pattern, cs.pix, (P.max_depth & 0xffffu) << 16, cs.sl));
    if (P.has_motion) st_nt(&S.time[i], cs.time);
  }
  // live slots of this segment = 1 + the largest valid k over the workgroup (valid k form a prefix)
  __shared__ uint32_t seg_max;
  if (threadIdx.x == 0) seg_max = 0;
  __syncthreads();
  if (seg_n) atomicMax(&seg_max, seg_n);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int b = 0; b < kBins; b++) {
      C->seg[0][blockIdx.x * kBins + b] = b == 0 ? seg_max : 0;
      C->seg[1][blockIdx.x * kBins + b] = 0;
    }
    C->shadow[blockIdx.x] = 0;
    if (blockIdx.x == 0) atomicAdd(&C->stats[0], (unsigned long long)total);  // camera_rays (tracer.rs:585)
  }
}
// ---- generate with the ROOT CULL (per-stage launches only; plan_launches holds the rule) ----
// On an open frame nearly every camera ray that escapes does so at the root: it tests the root's four child boxes,
// touches none and leaves (cornellbox 1080p: 44 % of the camera rays; 16 of 20 736 escaping rays get past the root). Such
// a ray used to be written here, fetched, set up and stepped once by the first extend, classified, queued and finished by
// a miss step of the first shade. Its whole traversal is four slab tests on wave-uniform data, and its origin and
// direction are in registers here: node_touched (dev_image.h — the engine's node step, expression for expression)
// decides, and a ray it calls a miss is finished on the spot with the miss step's arithmetic (escaped_to_sky) and the
// miss step's counters. The ray IS traced — its traversal is the root step, done where the ray is born — so closest_hit,
// escaped and the image keep their values. Survivors are appended to the front of the segment with the workgroup's LDS
// counter, as shade appends its survivors; a survivor's slot then no longer names its sample, so the compact form
// carries plane `d` as well (Params::cam_compact == 2). The slot loop is uniform: every wave appends in every round.
constexpr bool kRootCullBuild = kBins == 1 && !kRegenFirst;
__device__ __forceinline__ void generate_segment_cull(const Params &P, const PathSoA &S, Counters *C, uint32_t sample_begin,
                                                      uint32_t n_samples, uint32_t *sobol_tab /* kSobolLdsWords */, float4 *staging) {
  // the root's bounds and child words: wave-uniform, read once ahead of every store of this kernel (scalar loads)
  float bmin[3][4], bmax[3][4];
  uint32_t child[4];
  {
    const WideNode &root = P.scene.nodes[P.scene.root];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int l = 0; l < 4; l++) { bmin[a][l] = root.bmin[a][l]; bmax[a][l] = root.bmax[a][l]; }
#pragma unroll
    for (int l = 0; l < 4; l++) child[l] = root.child[l];
  }
  __shared__ uint32_t cull_ctr[2];  // survivors appended | camera rays finished here
  if (threadIdx.x < 2) cull_ctr[threadIdx.x] = 0;
  sobol_tables_init(sobol_tab);  // ends with a workgroup barrier
  const size_t total = (size_t)P.n_act * n_samples;
  const size_t seg0 = (size_t)blockIdx.x * kBins * P.seg_cap;  // camera rays are coherent as dealt: all in bin 0
  const bool compact = CRT_CAM_COMPACT_BUILD && P.cam_compact != 0;  // uniform
  uint32_t n_culled = 0;
  for (size_t k0 = 0; k0 < P.seg_cap; k0 += kBlock) {  // uniform: seg_cap is a multiple of the workgroup's width
    if (camera_slot_sample(k0) >= total) break;        // uniform: this round's first sample is past the end, so are all later ones
    const size_t g = camera_slot_sample(k0 + threadIdx.x);
    CameraSample cs;
    cs.o = splat(0.0f); cs.d = splat(0.0f); cs.time = 0.0f; cs.pattern = 0; cs.pix = 0; cs.sl = 0;
    bool keep = false;
    if (g < total) {  // the last round's ragged end: lanes past it append nothing
      cs = camera_sample(P, g, sample_begin, sobol_tab);
      // t_min / t_max as extend_segment's fetch sets them
      keep = node_touched(bmin, bmax, child, cs.o.x, cs.o.y, cs.o.z, cs.d.x, cs.d.y, cs.d.z, 0.001f, CRT_INF);
      if (!keep) {  // tracer.rs:1321-1342 with L = 0, beta = 1: the first shade's miss step
        const V3 L = escaped_to_sky(cs.d, splat(1.0f), splat(0.0f));
        st_nt(&staging[cs.sl * P.n_act + cs.pix], make_float4(L.x, L.y, L.z, 0.0f));
        n_culled++;
      }
    }
    const size_t i = seg0 + seg_append(keep, &cull_ctr[0]);
    if (keep) {
      const uint4 D = make_uint4(cs.pattern, cs.pix, (P.max_depth & 0xffffu) << 16, cs.sl);
      if (compact) {
        st_nt(&S.a[i], make_float4(cs.d.x, cs.d.y, cs.d.z, __uint_as_float(cs.pattern)));
        st_nt(&S.d[i], D);
      } else {
        st_nt(&S.a[i], make_float4(cs.o.x, cs.o.y, cs.o.z, cs.d.x));
        st_nt(&S.b[i], make_float4(cs.d.y, cs.d.z, 1.0f, 1.0f));
        st_nt(&S.d[i], D);
        if (P.has_motion) st_nt(&S.time[i], cs.time);
      }
    }
  }
  add_stat(&cull_ctr[1], n_culled);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int b = 0; b < kBins; b++) {
      C->seg[0][blockIdx.x * kBins + b] = b == 0 ? cull_ctr[0] : 0;
      C->seg[1][blockIdx.x * kBins + b] = 0;
    }
    C->shadow[blockIdx.x] = 0;
    if (blockIdx.x == 0) atomicAdd(&C->stats[0], (unsigned long long)total);  // camera_rays (tracer.rs:585)
    if (cull_ctr[1]) {  // closest_hit and escaped, at the indices shade's miss step feeds
      atomicAdd(&C->stats[1], (unsigned long long)cull_ctr[1]);
      atomicAdd(&C->stats[6], (unsigned long long)cull_ctr[1]);
    }
  }
}
__global__ __launch_bounds__(kBlock) void k_generate(Params P, PathSoA S, Counters *C, uint32_t sample_begin,
                                                     uint32_t n_samples, float4 *staging) {
  __shared__ uint32_t sobol_tab[kSobolLdsWords];
  if (kRootCullBuild && P.root_cull) generate_segment_cull(P, S, C, sample_begin, n_samples, sobol_tab, staging);  // uniform
  else generate_segment(P, S, C, sample_begin, n_samples, sobol_tab, false);
}

// ---- camera: generate, root cull and the camera rays' closest-hit traversal in ONE kernel (LaunchPlan::camera_trace) ----
// The 64 camera rays of a wave are 64 neighbouring pixels: they walk the tree together, so the pool engine's scheduler has
// nothing to repair on them, and a camera ray is in registers here. The sample loop is generate_segment_cull's — the same
// dealing, camera_sample, node_touched and escaped_to_sky; without the cull (Params::root_cull == 0) every sample goes on
// and keeps its slot, as in generate_segment — and a surviving ray is then traced in the lane that made it
// (traverse_camera.hip.h: the pool engine's node and packet steps, one ray per lane, the top of the tree and its packets
// read from LDS, a kCamStack-entry stack per lane in LDS) and its hit record written as extend_segment's emit writes it.
// Planes `a` and `d` go out for the first shade as before. What the loop does not handle — scalar leaf entries, a deeper
// stack — it leaves to the first extend: the ray's slot number goes to the segment's list in the other state buffer's
// plane `a`, the count to Counters::cam_defer, its hit record stays unwritten, and k_extend_deferred traces it from the
// root. Only the compact camera forms occur (plan_launches). mode: bit 0 every surviving ray is deferred, bits 8.. a
// stack limit below kCamStack (tests of the list and of the deferred instance).
constexpr int kCamLdsDwords = kCamWindow * kLdsNodeStride + kCamStack * kBlock;
static_assert((kSobolLdsWords + kCamLdsDwords) * 4 + 512 <= 40 * 1024, "four workgroups of k_camera per CU");
// TABLE: the sample loop reads the renderer's per-pixel table and steps a sample cursor (camera_pixel.hip.h,
// camera_sample_table) instead of calling camera_sample on the sample number; false: the loop as it was.
// ROOT_LDS: the cull reads the root node from the staged window every round (root_touched_lds) instead of holding its 28
// words in scalar registers the kernel parks in VGPR lanes; the plan asks for it only where the root is node 0, which
// stage_nodes always stages.
template <bool TABLE, bool ROOT_LDS>
__global__ __launch_bounds__(kBlock, 4) void k_camera(Params P, PathSoA S, uint32_t *defer_plane, HitSoA H, Counters *C,
                                                      uint32_t sample_begin, uint32_t n_samples, float4 *staging, uint32_t mode,
                                                      const PixelRec *pixel_table) {
  __shared__ uint32_t sobol_tab[kSobolLdsWords];
  __shared__ __attribute__((aligned(16))) uint32_t cam_lds[kCamLdsDwords];
  __shared__ uint32_t cam_ctr[3];  // survivors appended (live slots) | camera rays finished here | rays left to the first extend
  const bool cull = P.root_cull != 0;  // uniform
  float bmin[3][4] = {}, bmax[3][4] = {};
  uint32_t child[4] = {};
  if (!ROOT_LDS) {
    const WideNode &root = P.scene.nodes[P.scene.root];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int l = 0; l < 4; l++) { bmin[a][l] = root.bmin[a][l]; bmax[a][l] = root.bmax[a][l]; }
#pragma unroll
    for (int l = 0; l < 4; l++) child[l] = root.child[l];
  }
  if (threadIdx.x < 3) cam_ctr[threadIdx.x] = 0;
  uint32_t *lds_nodes = cam_lds;
  uint32_t *stk = cam_lds + kCamWindow * kLdsNodeStride + threadIdx.x;  // entry e of this lane: stk[e * kBlock]
  uint32_t n_lds_pk;
  const uint32_t n_lds = stage_nodes(P.scene, lds_nodes, kCamWindow, n_lds_pk);  // ends with a workgroup barrier
  sobol_tables_init(sobol_tab);                                                  // ... as does this
  const bool defer_all = (mode & 1u) != 0;
  const uint32_t want_stack = mode >> 8;
  const uint32_t pstack = (want_stack == 0 || want_stack > (uint32_t)kCamStack) ? (uint32_t)kCamStack : want_stack;
  const size_t total = (size_t)P.n_act * n_samples;
  const size_t seg0 = (size_t)blockIdx.x * kBins * P.seg_cap;
  uint32_t *list = defer_plane + 4 * seg0;  // 4 * seg_cap words of the segment's plane; at most seg_cap are used
  const V3 cam_o = ld3(P.camera.origin) + splat(0.0f);  // the pinhole camera's origin, as the compact form's readers take it
  uint32_t n_culled = 0, n_valid = 0;
  // TABLE: this lane's pixel slot and sample, round by round, and the pixel's record, loaded a round ahead
  SampleCursor at_g = {0, 0, 0, 0};
  uint4 rec0 = make_uint4(0, 0, 0, 0), rec1 = make_uint4(0, 0, 0, 0);
  if (TABLE) {
    at_g = sample_cursor(camera_slot_sample(threadIdx.x), (unsigned long long)gridDim.x * kBlock, P.n_act);
    pixel_rec_load(P, pixel_table, at_g.pix, rec0, rec1);
  }
  for (size_t k0 = 0; k0 < P.seg_cap; k0 += kBlock) {  // uniform: seg_cap is a multiple of the workgroup's width
    if (camera_slot_sample(k0) >= total) break;        // uniform
    const size_t g = camera_slot_sample(k0 + threadIdx.x);
    const uint32_t t_pix = at_g.pix, t_sl = at_g.sl;
    const uint4 t_rec0 = rec0, t_rec1 = rec1;
    if (TABLE) {  // the next round's record: its slot is below n_act whether or not that round exists
      sample_cursor_next(at_g, P.n_act);
      pixel_rec_load(P, pixel_table, at_g.pix, rec0, rec1);
    }
    CameraSample cs;
    cs.o = splat(0.0f); cs.d = splat(0.0f); cs.time = 0.0f; cs.pattern = 0; cs.pix = 0; cs.sl = 0;
    bool keep = false;
    if (g < total) {
      if (TABLE) cs = camera_sample_table(P, t_rec0, t_rec1, t_pix, t_sl, sample_begin, sobol_tab);
      else cs = camera_sample(P, g, sample_begin, sobol_tab);
      keep = true;
      n_valid = (uint32_t)(k0 + threadIdx.x) + 1;
      if (cull) {  // uniform
        keep = ROOT_LDS ? root_touched_lds(lds_nodes + (size_t)P.scene.root * kLdsNodeStride, cs.o, cs.d)
                        : node_touched(bmin, bmax, child, cs.o.x, cs.o.y, cs.o.z, cs.d.x, cs.d.y, cs.d.z, 0.001f, CRT_INF);
        if (!keep) {  // tracer.rs:1321-1342 with L = 0, beta = 1: the first shade's miss step
          const V3 L = escaped_to_sky(cs.d, splat(1.0f), splat(0.0f));
          st_nt(&staging[cs.sl * P.n_act + cs.pix], make_float4(L.x, L.y, L.z, 0.0f));
          n_culled++;
        }
      }
    }
    // under the cull the survivors are compacted; without it a sample keeps the slot it was dealt
    uint32_t at = (uint32_t)(k0 + threadIdx.x);
    if (cull) at = seg_append(keep, &cam_ctr[0]);  // uniform
    const size_t i = seg0 + at;
    int res = CAM_MISS;
    if (keep) {
      st_nt(&S.a[i], make_float4(cs.d.x, cs.d.y, cs.d.z, __uint_as_float(cs.pattern)));
      if (P.cam_compact == 2) st_nt(&S.d[i], make_uint4(cs.pattern, cs.pix, (P.max_depth & 0xffffu) << 16, cs.sl));  // uniform
      float t = 0.0f;
      uint32_t prim = kInvalid;
      res = defer_all ? (int)CAM_DEFER
                      : camera_trace(P.scene, lds_nodes, n_lds, n_lds_pk, stk, kBlock, pstack, 0.001f, CRT_INF, CRT_MASK_CAMERA,
                                     cam_o.x, cam_o.y, cam_o.z, cs.d.x, cs.d.y, cs.d.z, t, prim);
      if (res == CAM_HIT) {
        float4 h;
        uint32_t gw;
        camera_hit_record(P.scene, prim, t, cs.d.x, cs.d.y, cs.d.z, h, gw);
        st_hit(&H.h[i], h);
        st_hit(&H.geom[i], gw);
      } else if (res == CAM_MISS) {
        st_hit(&H.geom[i], kInvalid);
      }
    }
    const bool later = keep && res == CAM_DEFER;
    const uint32_t li = seg_append(later, &cam_ctr[2]);
    if (later) list[li] = (uint32_t)i;
  }
  add_stat(&cam_ctr[1], n_culled);
  if (!cull && n_valid) atomicMax(&cam_ctr[0], n_valid);  // live slots = 1 + the largest valid k (valid k form a prefix)
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int b = 0; b < kBins; b++) {
      C->seg[0][blockIdx.x * kBins + b] = b == 0 ? cam_ctr[0] : 0;
      C->seg[1][blockIdx.x * kBins + b] = 0;
    }
    C->shadow[blockIdx.x] = 0;
    C->cam_defer[blockIdx.x] = cam_ctr[2];
    if (blockIdx.x == 0) atomicAdd(&C->stats[0], (unsigned long long)total);  // camera_rays (tracer.rs:585)
    if (cam_ctr[1]) {  // closest_hit and escaped, at the indices shade's miss step feeds
      atomicAdd(&C->stats[1], (unsigned long long)cam_ctr[1]);
      atomicAdd(&C->stats[6], (unsigned long long)cam_ctr[1]);
    }
  }
}

// ---- extend: World::intersect (rt_world.rs:207-232) for every live path ----
// COMPACT: the 16-byte camera path form may occur (per-stage launches only: the fused kernel never sets it, and its
// fetch has no registers for the branch — 13 -> 27, 33 -> 97, 52 -> 122 spilled registers in the lit k_path instances).
// DEFER (k_extend_deferred): the rays are the camera rays k_camera left to this launch — their slot numbers come from the
// segment's list (defer_list: the other state buffer's plane `a`), their count from Counters::cam_defer.
// FACES (k_extend_faces): emit also keeps the hit's (prim_id, u, v, 0) in fplane, slot for slot beside H — what a
// per-face texture's lookup needs of the kernel's hit (rt_world.rs:212-218); COLD then carries u, v.
template <bool STATS, int WIDE, int COLD, bool COMPACT, bool DEFER = false, bool FACES = false>
__device__ __forceinline__ void extend_segment(const Params &P, const PathSoA &S, const HitSoA &H, Counters *C, int cur,
                                               int first, CrtTravStats *tstats, uint32_t *engine_lds,
                                               const uint32_t *defer_list = nullptr, uint4 *fplane = nullptr) {
  __shared__ uint32_t pre[kBins + 1];
  bins_prefix(&C->seg[cur][blockIdx.x * kBins], pre);
  const uint32_t n = DEFER ? C->cam_defer[blockIdx.x] : pre[kBins];
  if (n == 0) return;  // uniform per workgroup
  __shared__ uint32_t next;
  if (threadIdx.x == 0) next = 0;
  LaneStats st = {};
  uint32_t err = 0, done = 0;
  // every path of the first round is a camera ray, every later one an indirect ray (camera.rs:83, tracer.rs:1516-1519)
  const uint32_t mask = first ? CRT_MASK_CAMERA : CRT_MASK_INDIRECT;
  auto fetch = [&](bool want, RayIn &in) -> bool {
    uint32_t k;
    if (!lds_take(want, &next, n, k)) return false;
    const uint32_t i = DEFER ? defer_list[4 * (size_t)blockIdx.x * kBins * P.seg_cap + k] : bin_slot(k, pre, P.seg_cap);
    if (CRT_CAM_COMPACT_BUILD && COMPACT && first && P.cam_compact) {  // uniform: camera paths as 16-byte records (generate_segment)
      const float4 A = ld_nt(&S.a[i]);
      const V3 o = ld3(P.camera.origin) + splat(0.0f);
      in.ox = o.x; in.oy = o.y; in.oz = o.z; in.dx = A.x; in.dy = A.y; in.dz = A.z;
      in.time = 0.0f;
    } else {
      const float4 A = ld_nt(&S.a[i]), B = ld_nt(&S.b[i]);
      in.ox = A.x; in.oy = A.y; in.oz = A.z; in.dx = A.w; in.dy = B.x; in.dz = B.y;
      in.time = P.has_motion ? S.time[i] : 0.0f;
    }
    in.mask = mask; in.t_min = 0.001f; in.t_max = CRT_INF; in.slot = i;
    return true;
  };
  auto emit = [&](uint32_t i, bool hit, const Hit &h, float dx, float dy, float dz) {
    if (hit) {
      const bool front = dot3(dx, dy, dz, h.nx, h.ny, h.nz) < 0.0f;  // scene.rs:356-359
      st_hit(&H.h[i], make_float4(h.t, front ? h.nx : -h.nx, front ? h.ny : -h.ny, front ? h.nz : -h.nz));
      st_hit(&H.geom[i], h.geom | (front ? 0x80000000u : 0u));
      if (FACES) fplane[i] = make_uint4(h.prim, __float_as_uint(h.u), __float_as_uint(h.v), 0u);
    } else {
      st_hit(&H.geom[i], kInvalid);
    }
    done++;
  };
  // the four-wave kernels keep no mask plane: every ray of the launch carries `mask` (UMASK, traverse_pool.hip.h)
  run_traversal<false, STATS, WIDE, COLD, WIDE != 0>(P.scene, engine_lds, 0.001f, err, st, fetch, emit, mask);
  if (err) atomicOr(&C->err, err);
  if (STATS) flush_stats(st, tstats, done);
}
// WIDE: the four-workgroups-per-CU split of the engine (traverse_pool.hip.h), the per-stage pipeline of flat scenes.
// COLD: the cold per-ray state the scene can need (DevScene::cold; the hit record carries no u, v, so a scene needs
// kColdUV only for shading normals): 0 for flat-shaded static triangle scenes, kColdNormal with spheres or nested
// instances, kColdAll otherwise and for the stats build.
template <bool STATS, int WIDE, int COLD>
__global__ __launch_bounds__(kBlock, WIDE ? 4 : CRT_EXTEND_WAVES) void k_extend(Params P, PathSoA S, HitSoA H, Counters *C, int cur,
                                                                     int first, CrtTravStats *tstats) {
  __shared__ __attribute__((aligned(16))) uint32_t engine_lds[WIDE ? kEngineLdsWide : kEngineLdsDwords];
  extend_segment<STATS, WIDE, COLD, true>(P, S, H, C, cur, first, tstats, engine_lds);
}
// The first extend behind k_camera: the same engine instance over the segment's list of deferred camera rays (usually a
// few per cent of the segment, often none). A kernel of its own, so that k_extend — every later bounce — is untouched.
template <bool STATS, int WIDE, int COLD>
__global__ __launch_bounds__(kBlock, WIDE ? 4 : CRT_EXTEND_WAVES) void k_extend_deferred(Params P, PathSoA S, HitSoA H, Counters *C, int cur,
                                                                              int first, CrtTravStats *tstats, const uint32_t *defer_list) {
  __shared__ __attribute__((aligned(16))) uint32_t engine_lds[WIDE ? kEngineLdsWide : kEngineLdsDwords];
  extend_segment<STATS, WIDE, COLD, true, true>(P, S, H, C, cur, first, tstats, engine_lds, defer_list);
}

// The extend of textured renders (LaunchPlan::faces): the engine instance the image runs, with the cold state that holds
// u, v. A kernel of its own, so that k_extend is untouched.
template <int WIDE, int COLD>
__global__ __launch_bounds__(kBlock, WIDE ? 4 : CRT_EXTEND_WAVES) void k_extend_faces(Params P, PathSoA S, HitSoA H, Counters *C, int cur,
                                                                           int first, CrtTravStats *tstats, uint4 *fplane) {
  static_assert((COLD & (int)kColdUV) != 0, "the face lookup reads the hit's barycentrics");
  __shared__ __attribute__((aligned(16))) uint32_t engine_lds[WIDE ? kEngineLdsWide : kEngineLdsDwords];
  extend_segment<false, WIDE, COLD, true, false, true>(P, S, H, C, cur, first, tstats, engine_lds, nullptr, fplane);
}

// The view a vertex's scatter and evals run through. Unbound instances: the table's own view, the very object the vertex
// code named before textures existed (view_of hands its reference back). FACES: a MatFace beside it — the record with
// the texel of the hit's face in the place of base_color where the geometry has a face map, the material a texture and
// the face resolves (openpbr.rs:1011-1024); every other lane carries the record's own colour, which gives the untextured
// view's bits. Emission reads the table's view in either form: the authored colour, as upstream.
template <bool FACES> struct FacesTag {};
struct NoFaceView {};
template <class MV>
__device__ __forceinline__ NoFaceView face_view(FacesTag<false>, const MV &, const FaceView *, const uint4 *, uint32_t, uint32_t) { return NoFaceView{}; }
template <class MV>
__device__ __forceinline__ MatFace face_view(FacesTag<true>, const MV &mv, const FaceView *FV, const uint4 *fplane, uint32_t i, uint32_t geom) {
  const CrtMaterial &m = mv.raw();
  V3 base = ld3(m.base_color);
  if (geom < FV->n_geoms && FV->geoms[geom] != kFaceNone) {  // the geometry has a binding: read the hit's record
    const uint4 r = fplane[i];
    const FaceCoord c = face_resolve(*FV, geom, r.x, __uint_as_float(r.y), __uint_as_float(r.z));
    const uint32_t tex = geom < FV->n_materials ? FV->material_texture[geom] : kFaceNone;
    if (tex != kFaceNone && c.face != kNoFace) base = face_texture_eval(*FV, tex, c.face, c.u, c.v);
  }
  return MatFace{m, BaseTexel{base}};
}
template <class MV>
__device__ __forceinline__ const MV &view_of(const MV &mv, const NoFaceView &) { return mv; }
template <class MV>
__device__ __forceinline__ const MatFace &view_of(const MV &, const MatFace &fv) { return fv; }

// ---- shade: one iteration of trace_path's loop body for every live path (tracer.rs:1118-1530) ----
// LIT: the light list is not empty. Unlit scenes (cornellbox, the bench scene: sky only) run an instance without the
// light-sampling block, its second BSDF evaluation, the emitter MIS weights and the previous-vertex plane — code they
// never execute, but whose registers and scalar constants the fused kernel otherwise carries through every bounce
// (cornellbox +1.3 %, MedCity +2 %, profiles/README.md). With lights present the strategy is checked at run time.
// MATS: what the scene's material table holds — 0 simple (no coat, fuzz, thin film, transmission, subsurface anywhere:
// the OpenPBR code is instantiated without those arms, shade.hip.h), 1 general, 2 general with interior media.
// CRT_SHADE_STAMPS=1 builds (measurement only, never shipped): the four-wave shade kernels stamp the parts of their loop
// with the cycle counter and sum wave cycles into Counters::cls_waves / cls_lanes, eight slots read and cleared by
// crt_renderer_shade_class_stats. A load's wait is made explicit (vmcnt(0)) before its stamp, so the build is slower:
// read ratios. shade_segment: [0] CLASSIFY load wait, [1] CLASSIFY work, [2] barriers, [3] vertex load wait,
// [4] vertex compute, [5] stores, [6] iterations, [7] CLASSIFY rounds.
#ifndef CRT_SHADE_STAMPS
#define CRT_SHADE_STAMPS 0
#endif
// INF: 0 no light at infinity in the list | 1 distant lights and uniform domes | 2 mapped domes too (k_shade_env)
// VOL: the instances of volume renders (k_shade_vol). k_volume has run between extend and this stage: segment transmittance
// and emission are in beta and L already, and a path that scattered inside a region arrives as a finished phase vertex
// behind a kVolScatter hit word — its values are loaded into the variables of the tail below, which compacts, queues the
// shadow request and stages as for any vertex; the vertex code is skipped. Every shadow request's K_NEE_SHADOW seed goes
// to qseed (k_shadow_volume walks the segment with it).
// GUIDED: the instances of guided renders (k_shade_guided), render_pass(.., Some(&GuidingContext{field, training: false}))
// — the guided-forward form of DESIGN.md §2. At a surface vertex with a previous vertex (tracer.rs:1386: never the camera
// vertex, never the vertex behind an interior-medium scatter) ONE spatial descent finds the D-tree governing rec.p; where
// that tree is trained the NEE weight's bounce pdf is the mixture (tracer.rs:1432-1440) and the bounce is
// sample_bounce_direction (tracer.rs:777-826, guide_sample_bounce_at), whose mixture pdf travels on as n_ppdf. The view GV
// is the kernel's argument: alpha, bounds, counts and array bases are wave-uniform. No loop, LDS word or barrier is new.
template <int MATS, int INF, bool LIT, int ARENA, bool DRV, bool VOL = false, bool FACES = false, bool GUIDED = false>
__device__ __forceinline__ void shade_segment(const Params &P, const PathSoA &S, const PathSoA &N, const HitSoA &H,
                                              const ShadowSoA &Q, Counters *C, int cur, float4 *staging,
                                              uint32_t *sobol_tab /* ARENA dwords: Sobol tables, then the material table */,
                                              bool first /* camera paths whose plane c was not written (generate_segment) */,
                                              bool all_pending = false /* no CLASSIFY pass: every path takes the vertex step */,
                                              uint32_t *qseed = nullptr /* VOL: one word per shadow-queue slot */,
                                              const FaceView *FV = nullptr, const uint4 *fplane = nullptr /* FACES */,
                                              const GuideView *GV = nullptr /* GUIDED */) {
  constexpr bool MEDIA = MATS == 2, SIMPLE = MATS == 0;
  static_assert(!GUIDED || (!VOL && !FACES && !DRV), "guided renders: raw records, neither volumes nor textures");
  static_assert(SIMPLE || !DRV, "the derived record covers what a simple-material table reads (shade.hip.h)");
  typedef MatTable<DRV> Table;
  // Two of round 3's forms are compiled only into the instances that have registers to spare: the lit four-wave shade
  // kernel sits at its 128-register limit with 17 spilled, and the few branches of either form cost it 3.6 % / 0.9 %
  // (cornellbox_guided) where the unlit one gains 1 % (profiles/README.md). The host sets Params::cam_compact for
  // unlit scenes only and runs a deduplicated table (Params::mat_index) through the three-wave shade kernel.
  constexpr bool COMPACT = CRT_CAM_COMPACT_BUILD && !LIT;
  constexpr bool COMPACT_D = COMPACT && SIMPLE;  // ... with plane d read back (root cull): the simple-material instances only
  constexpr bool MAT_INDEX = CRT_MAT_INDEX_BUILD && ARENA != kArenaWide;
  __shared__ uint32_t lds_ctr[10];  // [1] shadow requests, [2..8] statistics
  __shared__ uint32_t out_n[kBins];  // survivors per direction bin
  __shared__ uint32_t pre[kBins + 1];
  bins_prefix(&C->seg[cur][blockIdx.x * kBins], pre);
  const uint32_t n = pre[kBins];
  if (n == 0) {  // nothing lives in this segment (uniform per workgroup): publish empty outputs and leave
    if (threadIdx.x < kBins) C->seg[1 - cur][blockIdx.x * kBins + threadIdx.x] = 0;
    if (threadIdx.x == 0) C->shadow[blockIdx.x] = 0;
    return;
  }
  if (threadIdx.x < 10) lds_ctr[threadIdx.x] = 0;
  if (threadIdx.x < kBins) out_n[threadIdx.x] = 0;
  sobol_tables_init(sobol_tab);  // ends with a workgroup barrier
  // The vertex code reads its material record a field at a time, where each lobe needs it: two dozen dependent
  // round trips to L2 per vertex. A table that fits the rest of the arena is staged in LDS once per call instead
  // (generic pointer: the reads become FLAT loads served by LDS); larger tables stay in global memory.
  // (Either table: a DevMaterial has the size of a CrtMaterial, so mat_lds_max holds for both.)
  const typename Table::Rec *mats = Table::of(P);
  if (P.n_materials <= (uint32_t)mat_lds_max(ARENA)) {
    uint32_t *dst = sobol_tab + kSobolLdsWords;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(mats);
    const uint32_t words = P.n_materials * (uint32_t)(sizeof(CrtMaterial) / 4);
    for (uint32_t w = threadIdx.x; w < words; w += kBlock) dst[w] = src[w];
    mats = reinterpret_cast<const typename Table::Rec *>(dst);
    __syncthreads();
  }
  const uint32_t seg0 = blockIdx.x * P.seg_cap;  // shadow queue: one unbinned segment per workgroup
  const uint32_t n_lights = LIT ? P.n_lights : 0u;
  uint32_t s_closest = 0, s_shadow = 0, s_vertices = 0, s_rr_t = 0, s_rr_k = 0, s_esc = 0, s_depth = 0;
  // Two kinds of work per path: a ray that escaped just adds the sky and ends (cheap), everything else runs the full
  // vertex (expensive). Mixed in one wave the escaped lanes would idle through the vertex code — a third of the
  // rays on an open scene — so the segment is swept in two interleaved steps: CLASSIFY takes the next 256 paths,
  // finishes the escaped ones on the spot and appends the others to a ring of pending indices in LDS; SHADE takes
  // 256 pending paths at a time (fewer only when the input is exhausted), so the vertex code runs on full waves.
  // PARTITION (scenes with more than one material class): the pending vertices are kept in one ring PER CLASS and a
  // SHADE step takes its 256 from ONE ring — the fullest — so all four waves of the step run one class's arms. The
  // class comes from a byte table by geom_id (LDS when it fits). Per-path arithmetic does not depend on which lanes
  // share a wave, and every output slot is private to its path, so images and counters do not change.
  uint32_t *ring = sobol_tab + ARENA - kRingDwords;               // [kClasses][kRing]
  uint8_t *cls_lds = reinterpret_cast<uint8_t *>(ring) - kClassLdsMax;
  __shared__ uint32_t ring_tail[kClasses];  // entries ever appended, per class (heads are tracked in registers: uniform)
  const bool part = P.partition != 0;
  const bool cls_in_lds = part && P.n_materials <= (uint32_t)kClassLdsMax;
  if (threadIdx.x < kClasses) ring_tail[threadIdx.x] = 0;
  if (cls_in_lds)
    for (uint32_t g = threadIdx.x; g < P.n_materials; g += kBlock) cls_lds[g] = P.mat_class[g];
  __syncthreads();
  uint32_t next_in = 0;
  uint32_t head[kClasses], tail[kClasses];
  constexpr bool STAMPS = CRT_SHADE_STAMPS != 0 && ARENA == kArenaWide;
  unsigned long long t_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t0 = STAMPS ? __builtin_readcyclecounter() : 0ull;
  auto lap = [&](int slot, bool drain) {
    if (STAMPS) {
      if (drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned long long t = __builtin_readcyclecounter();
      t_acc[slot] += t - t0;
      t0 = t;
    }
  };
#pragma unroll
  for (int c = 0; c < kClasses; c++) head[c] = 0;
  for (;;) {
#pragma unroll
    for (int c = 0; c < kClasses; c++) tail[c] = ring_tail[c];  // uniform: read between two barriers, nobody appends meanwhile
    __syncthreads();
    lap(2, false);
    auto most_pending = [&](int &c_best) {
      uint32_t best = tail[0] - head[0];
      c_best = 0;
#pragma unroll
      for (int c = 1; c < kClasses; c++)
        if (tail[c] - head[c] > best) { best = tail[c] - head[c]; c_best = c; }
      return best;
    };
    int c_sel;
    // ---- CLASSIFY while no class has a workgroup's worth of vertices pending and input remains ----
    while (most_pending(c_sel) < (uint32_t)kBlock && next_in < n) {
      const uint32_t k_c = next_in + threadIdx.x;
      next_in += kBlock;
      bool pending = false;
      uint32_t cls = 0;
      // all_pending (per-stage pipeline, bounces after the first, one material class): CLASSIFY reads nothing and sends
      // every path to the vertex step, whose own escaped arm adds the sky (same expression, same counters). The escaped
      // lanes then idle through the vertex code of their wave — a quarter to a third of the lanes at bounces 1-3 of the
      // bench — but the path state is read ONCE: CLASSIFY's 68 bytes per path were read a second time, from HBM, by the
      // vertex step of every path that had hit something.
      if (all_pending && !part) pending = k_c < n;
      else if (k_c < n) {
        const uint32_t i_c = bin_slot(k_c, pre, P.seg_cap);
        const uint32_t hg = H.geom[i_c];
        // the escaped arm's operands are requested together with the classification's (one memory round trip, not
        // two); for a path that hit something they are loaded again by the vertex step, from L2. (Requested for the
        // escaped lanes only — 48 B less per hit path — the per-stage shade is 1.5 % slower: profiles/README.md.)
        uint4 D;
        float4 A, B, Cc = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
        if (COMPACT && first && P.cam_compact) {  // uniform
          float4 a = S.a[i_c];
          if (COMPACT_D && P.cam_compact == 2) D = S.d[i_c];  // uniform: the root cull's survivors carry their pixel and sample
          asm volatile("" : "+v"(a.x));
          if (STAMPS) asm volatile("s_waitcnt vmcnt(0)" : "+v"(a.x) : : "memory");
          compact_camera_path<COMPACT_D>(P, k_c, a, A, B, D);
        } else if (!(kRegenFirst && first)) {
          D = S.d[i_c]; A = S.a[i_c]; B = S.b[i_c];
          if (!first) Cc = S.c[i_c];
          asm volatile("" : "+v"(A.x), "+v"(B.x), "+v"(Cc.x));
          if (STAMPS) asm volatile("s_waitcnt vmcnt(0)" : "+v"(A.x), "+v"(D.x) : : "memory");
        } else {
          // a camera path: only the direction (escaped rays) and the film slot are needed here, and both follow from the
          // slot number; nothing of the path state is read (generate_segment)
          D = make_uint4(0u, 0u, (P.max_depth & 0xffffu) << 16, 0u);
          A = make_float4(0.0f, 0.0f, 0.0f, 0.0f); B = make_float4(0.0f, 0.0f, 1.0f, 1.0f);
          if (hg == kInvalid && P.max_depth > 0) {
            const CameraSample cs = camera_sample(P, camera_slot_sample(k_c), P.sample_begin, sobol_tab);
            A.w = cs.d.x; B.x = cs.d.y; B.y = cs.d.z;
            D.y = cs.pix; D.w = cs.sl;
          }
        }
        lap(0, false);
        const int remaining = (int)(D.z >> 16);
        const bool carries_medium = MEDIA && (D.w >> kMediumShift) != 0;
        if (!INF && hg == kInvalid && remaining > 0 && !carries_medium) {
          // tracer.rs:1321-1342: the path ends on the sky gradient. (With lights at infinity — INF — escaped rays
          // take the full vertex step instead: their background is a loop over the light list.)
          const V3 rd = v3(A.w, B.x, B.y), beta = v3(B.z, B.w, Cc.x);
          V3 L = v3(Cc.y, Cc.z, Cc.w);
          s_closest++;
          s_esc++;
          L = escaped_to_sky(rd, beta, L);
          st_nt(&staging[(D.w & 0xffffu) * P.n_act + D.y], make_float4(L.x, L.y, L.z, 0.0f));
        } else {
          pending = true;
          if (part && hg != kInvalid && !(VOL && vol_scatter_word(hg))) {
            const uint32_t g = hg & 0x7fffffffu;
            const uint32_t mi_c = (MAT_INDEX && P.mat_index) ? (uint32_t)P.mat_index[g] : g;
            cls = cls_in_lds ? cls_lds[mi_c] : P.mat_class[mi_c];
          }
        }
      }
      if (part) {
#pragma unroll
        for (int c = 0; c < kClasses; c++) {
          const bool mine = pending && cls == (uint32_t)c;
          const uint32_t at = seg_append(mine, &ring_tail[c]);
          if (mine) ring[c * kRing + at % kRing] = k_c;
        }
      } else {
        const uint32_t at = seg_append(pending, &ring_tail[0]);
        if (pending) ring[at % kRing] = k_c;
      }
      lap(1, false);
      __syncthreads();
#pragma unroll
      for (int c = 0; c < kClasses; c++) tail[c] = ring_tail[c];
      __syncthreads();
      lap(2, false);
      if (STAMPS) t_acc[7]++;
    }
    const uint32_t avail = most_pending(c_sel);
    if (avail == 0) break;  // uniform: input exhausted and nothing pending
    // ---- SHADE up to a workgroup's worth of pending vertices of the fullest class ----
    const uint32_t take = avail < (uint32_t)kBlock ? avail : (uint32_t)kBlock;
    const bool active = threadIdx.x < take;
    uint32_t head_sel = head[0];
#pragma unroll
    for (int c = 1; c < kClasses; c++) head_sel = c_sel == c ? head[c] : head_sel;
    const uint32_t k_in = active ? ring[c_sel * kRing + (head_sel + threadIdx.x) % kRing] : 0;
#pragma unroll
    for (int c = 0; c < kClasses; c++) head[c] += c_sel == c ? take : 0u;
    const uint32_t i = active ? bin_slot(k_in, pre, P.seg_cap) : 0;
    bool alive = false, want_shadow = false;
    V3 L = splat(0.0f), beta = splat(1.0f);
    V3 n_o = splat(0.0f), n_d = splat(0.0f), sh_d = splat(0.0f), sh_c = splat(0.0f), hit_p = splat(0.0f);
    float n_ppdf = 0.0f, sh_tmax = 0.0f, time = 0.0f;
    uint32_t meta = 0, aux = 0, pix = 0, pattern = 0, n_med = 0;
    bool n_delta = false, n_prev_valid = true;
    if (active) {
      float4 A, B, Cc = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
      uint4 D;
      if (COMPACT && first && P.cam_compact) {  // uniform
        if (COMPACT_D && P.cam_compact == 2) D = S.d[i];  // uniform (root cull)
        compact_camera_path<COMPACT_D>(P, k_in, S.a[i], A, B, D);
        time = 0.0f;
      } else if (!(kRegenFirst && first)) {
        A = S.a[i]; B = S.b[i]; D = S.d[i];
        if (!first) Cc = S.c[i];
        time = P.has_motion ? S.time[i] : 0.0f;
      } else {  // a camera path: the sample is worked out again from the slot number (generate_segment)
        const CameraSample cs = camera_sample(P, camera_slot_sample(k_in), P.sample_begin, sobol_tab);
        A = make_float4(cs.o.x, cs.o.y, cs.o.z, cs.d.x); B = make_float4(cs.d.y, cs.d.z, 1.0f, 1.0f);
        D = make_uint4(cs.pattern, cs.pix, (P.max_depth & 0xffffu) << 16, cs.sl);
        time = cs.time;
      }
      const V3 ro = v3(A.x, A.y, A.z), rd = v3(A.w, B.x, B.y);
      beta = v3(B.z, B.w, Cc.x);
      L = v3(Cc.y, Cc.z, Cc.w);
      pattern = D.x; pix = D.y; meta = D.z; aux = D.w;
      const uint32_t n_rec = meta & 0xffffu;
      const int remaining = (int)(meta >> 16);
      const bool prev_valid = (aux & kPrevValid) != 0, prev_delta = (aux & kPrevDelta) != 0;
      const uint32_t med_id = MEDIA ? aux >> kMediumShift : 0u;  // Ray::medium: the interior this segment travels in
      DevMedium med;
      med.present = 0; med.scattering = 0;
      if (MEDIA && med_id) med = P.media_by_id[med_id - 1];
      n_med = med_id;
      const uint32_t hg = H.geom[i];
      const bool vol_vertex = VOL && vol_scatter_word(hg);  // a phase vertex k_volume prepared: no surface, no material
      const bool has_hit = hg != kInvalid && !vol_vertex;
      const uint32_t geom = hg & 0x7fffffffu;
      // the material record's index: the geometry id, or (deduplicated tables) one 2-byte load away
      const uint32_t mat_i = (MAT_INDEX && has_hit && P.mat_index) ? (uint32_t)P.mat_index[geom] : geom;
      if (P.class_stats) {  // uniform; diagnostic only
        const uint32_t my = has_hit ? (uint32_t)P.mat_class[(MAT_INDEX && P.mat_index) ? (uint32_t)P.mat_index[geom] : geom] : 0u;
#pragma unroll
        for (int c = 0; c < kClasses; c++) {
          const unsigned long long m = __ballot(my == (uint32_t)c);
          if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) {
            atomicAdd(&C->cls_waves[c], 1ull);
            atomicAdd(&C->cls_lanes[c], (unsigned long long)__popcll(m));
          }
        }
      }
      HitRec rec;
      rec.front_face = ((hg >> 31) & 1u) != 0;
      rec.t = 0.0f; rec.normal = splat(0.0f); rec.p = splat(0.0f);
      if (has_hit) {
        const float4 hh = H.h[i];
        rec.t = hh.x;
        rec.normal = v3(hh.y, hh.z, hh.w);
        rec.p = ro + rd * rec.t;  // ray.at(t), rt_world.rs:221
      }
      hit_p = rec.p;
      if (STAMPS) asm volatile("" : "+v"(hit_p.x), "+v"(beta.x), "+v"(L.x), "+v"(pattern));
      lap(3, true);

      // bounce_emission_weight (tracer.rs:930-953). A previous bounce exists only where scatter returned a
      // sample, i.e. where eval is available, so the "eval is None" arm reduces to the delta flag.
      auto emission_weight = [&]() -> float {
        if (prev_delta) return 1.0f;
        for (uint32_t k = 0; k < n_lights; k++) {  // LightList::find_by_geom, light.rs:436-440
          if (P.lights[k].geom_id == geom) {
            const float4 E = S.e[i];
            const V3 from = v3(E.x, E.y, E.z);
            const float light_pdf = rmax(solid_angle_pdf(P.lights[k], from, rec.p) / (float)n_lights, 1e-6f);
            return bounce_weight(P.strategy, E.w, light_pdf);
          }
        }
        return 1.0f;
      };

      if (VOL && vol_vertex) {  // tracer.rs:1192-1249, computed by k_volume (which also counted it): the tail's inputs
        alive = (hg & 1u) != 0;
        n_o = ro; n_d = rd; hit_p = ro;  // the new ray leaves the scatter point; beta, L, n_med are what was loaded
        n_delta = false; n_prev_valid = true;
        if (LIT) {
          const float4 E = S.e[i], hq = H.h[i];
          n_ppdf = E.w;
          want_shadow = (hg & 2u) != 0;
          sh_c = v3(E.x, E.y, E.z); sh_d = v3(hq.x, hq.y, hq.z); sh_tmax = hq.w;
        }
      } else if (remaining <= 0) {  // tracer.rs:1123-1149: depth exhausted, last-vertex emission only
        s_depth++;
        if (prev_valid) {
          s_closest++;
          if (has_hit) {
            const auto mat = Table::view(mats, P, mat_i);
            const float cos_o = fabs_(dot(normalize(rd), rec.normal));
            V3 emitted = mat_emitted_directional<SIMPLE>(mat, cos_o);
            if (len2(emitted) > 0.0f) {
              if (MEDIA && med.present) emitted = emitted * medium_transmittance(med, rec.t);  // tracer.rs:1134-1136
              L = L + beta * (emitted * emission_weight());
            }
          }
        }
      } else {
        s_closest++;
        const Sampler vdom = new_domain(Sampler{pattern, P.sample_begin + (aux & 0xffffu)}, (int)n_rec);  // :1121
        // free-flight candidate in a scattering carried medium (tracer.rs:1159-1165)
        float t_med = CRT_INF;
        if (MEDIA && med.present && med.scattering) t_med = -(log_det(draw_rnd1(new_domain(vdom, K_MEDIUM)))) / med.sigma_bar;
        const float t_surf = has_hit ? rec.t : CRT_INF;
        if (MEDIA && t_med < t_surf) {  // === carried-medium scatter vertex (tracer.rs:1256-1319): no NEE, next emission in full ===
          const V3 pos = ro + rd * t_med;
          float phase_uv[4];
          draw_sample4(new_domain(vdom, K_PHASE), phase_uv, sobol_tab);
          const V3 dir = sample_henyey_greenstein(normalize(rd), med.g, phase_uv[0], phase_uv[1]);
          const V3 factor = (ld3(med.sigma_s) / med.sigma_bar) * medium_chromatic(med, t_med);
          beta = beta * (splat(1.0f) * factor);
          bool survived = true;
          if (n_rec >= (uint32_t)kRrStartBounce) {
            s_rr_t++;
            const float p_survive = rclamp(max_elem(beta), kRrMinProb, 1.0f);
            if (p_survive < 1.0f) {
              if (draw_rnd1(new_domain(vdom, K_RR)) >= p_survive) {
                survived = false;
                s_rr_k++;
              } else {
                beta = beta / p_survive;
              }
            }
          }
          s_vertices++;
          if (survived) {
            alive = true;
            n_o = pos; n_d = dir; n_ppdf = 0.0f; n_delta = false; n_prev_valid = false;  // same medium: n_med stays
          }
        } else if (!has_hit) {  // tracer.rs:1321-1342 (rays that carried a medium out of the scene end here)
          s_esc++;
          const V3 unit_direction = normalize(rd);
          // plane e exists from the first bounce on (generate does not write it): a camera path never loads it
          const bool competing = prev_valid && !prev_delta;
          float prev_pdf = 0.0f;
          if (INF && competing) prev_pdf = S.e[i].w;
          const V3 background = INF ? escaped_background<INF == 2>(P.lights, n_lights, P.strategy, unit_direction, competing, prev_pdf, P.envs)
                                    : splat(0.0f) + sky_gradient(unit_direction);
          L = L + beta * background;
        } else {
          const auto mat = Table::view(mats, P, mat_i);
          const auto fmat = face_view(FacesTag<FACES>{}, mat, FV, fplane, i, geom);
          // tracer.rs:1352-1361: a scattering medium already paid e^{-sigma_bar t} through the free-flight
          // competition, only the chromatic correction remains; a clear one keeps pure Beer-Lambert.
          V3 atten = splat(1.0f);
          if (MEDIA && med.present) atten = splat(1.0f) * (med.scattering ? medium_chromatic(med, rec.t) : medium_transmittance(med, rec.t));
          const float cos_o = fabs_(dot(normalize(rd), rec.normal));
          const V3 emitted = mat_emitted_directional<SIMPLE>(mat, cos_o);
          V3 emit_here = splat(0.0f);
          if (prev_valid) {  // tracer.rs:1372-1381
            if (len2(emitted) > 0.0f) L = L + beta * ((atten * emitted) * emission_weight());
          } else {
            emit_here = emitted;
          }
          const V3 ba = beta * atten;
          // guiding_here (tracer.rs:1386) and the one descent NEE and the bounce share
          uint32_t g_root = kGuideNoChild;
          bool g_trained = false;
          if (GUIDED && prev_valid) {
            g_root = guide_dtree_at(*GV, rec.p);
            g_trained = guide_trained(*GV, g_root);
          }

          // === 1. direct lighting by light sampling (tracer.rs:1394-1445) ===
          if (LIT && P.strategy != CRT_STRATEGY_BSDF && n_lights > 0) {
            float nee_s[4];
            draw_sample4(new_domain(vdom, K_NEE), nee_s, sobol_tab);
            uint32_t li = (uint32_t)(nee_s[0] * (float)n_lights);  // LightList::pick, light.rs:421-429
            if (li > n_lights - 1) li = n_lights - 1;
            const CrtLight &light = P.lights[li];
            LightSample ls;
            if (light_sample_li_env<INF>(light, P.envs, rec.p, nee_s[1], nee_s[2], ls)) {
              s_shadow++;  // the reference traces the shadow ray before it evaluates the BSDF (tracer.rs:1412-1425)
              want_shadow = true;
              sh_d = ls.direction;
              sh_tmax = ls.distance - 0.001f;
              const float cosine = fabs_(dot(rec.normal, ls.direction));
              const float light_pdf = rmax(ls.pdf / (float)n_lights, 1e-6f);
              V3 brdf_value; float brdf_pdf;
              V3 nee = splat(0.0f);
              if (mat_eval<SIMPLE>(view_of(mat, fmat), rd, rec, ls.direction, brdf_value, brdf_pdf)) {
                // the competing strategy is the bounce sampler: the guide / BSDF mixture where the field is trained here
                if (GUIDED && g_trained) brdf_pdf = GV->alpha * guide_field_pdf_at(*GV, g_root, ls.direction) + (1.0f - GV->alpha) * brdf_pdf;
                const float weight = light_weight(P.strategy, light_pdf, brdf_pdf);
                V3 c = (ls.radiance * brdf_value) * cosine;
                c = c * splat(1.0f);  // shadow_tr == ONE when unoccluded
                nee = nee + (c * weight) / light_pdf;
              }
              sh_c = ba * nee;  // added to L by the shadow stage iff the segment is unoccluded
            }
          }
          L = L + ba * emit_here;

          // === 2. indirect lighting by BSDF sampling (tracer.rs:1459-1523) ===
          Scatter sample;
          bool scattered;
          if (GUIDED) {  // off the vertex domain: K_BSDF and K_GUIDE are derived inside (an untrained vertex: mat_scatter on K_BSDF)
            uint32_t g_flags;
            scattered = guide_sample_bounce_at<SIMPLE, false>(*GV, g_root, g_trained, mat.raw(), rd, rec, vdom, sample, g_flags, sobol_tab);
          } else {
            scattered = mat_scatter<SIMPLE>(view_of(mat, fmat), rd, rec, new_domain(vdom, K_BSDF), sample, sobol_tab);
          }
          if (scattered) {
            const V3 dir = normalize(sample.dir);
            const float cosine = sample.delta ? 1.0f : fabs_(dot(rec.normal, dir));
            const V3 factor = (sample.value * cosine) / sample.pdf;
            beta = beta * (atten * factor);
            bool survived = true;
            if (n_rec >= (uint32_t)kRrStartBounce) {
              s_rr_t++;
              const float p_survive = rclamp(max_elem(beta), kRrMinProb, 1.0f);
              if (p_survive < 1.0f) {
                if (draw_rnd1(new_domain(vdom, K_RR)) >= p_survive) {
                  survived = false;
                  s_rr_k++;
                } else {
                  beta = beta / p_survive;
                }
              }
            }
            if (survived) {
              alive = true;
              n_o = sample.origin; n_d = sample.dir; n_ppdf = sample.pdf; n_delta = sample.delta;
              // materials build the ray: it carries the interior only when it refracts into the front face
              n_med = (MEDIA && sample.medium) ? P.media[mat_i].id : 0u;
            }
          }
          s_vertices++;
        }
      }
    }

    lap(4, false);
    // ---- wave-level compaction: survivors go to the other state buffer, finished paths to the film ----
    uint32_t j = 0;
    {
      const uint32_t my_bin = dir_bin(n_d.x, n_d.y, n_d.z);
#pragma unroll
      for (int b = 0; b < kBins; b++) {
        const bool mine = alive && my_bin == (uint32_t)b;
        const uint32_t pos = seg_append(mine, &out_n[b]);
        if (mine) j = (blockIdx.x * kBins + b) * P.seg_cap + pos;
      }
    }
    const uint32_t sl = aux & 0xffffu;
    const uint32_t film_idx = sl * P.n_act + pix;
    if (alive) {
      st_nt(&N.a[j], make_float4(n_o.x, n_o.y, n_o.z, n_d.x));
      st_nt(&N.b[j], make_float4(n_d.y, n_d.z, beta.x, beta.y));
      st_nt(&N.c[j], make_float4(beta.z, L.x, L.y, L.z));
      st_nt(&N.d[j], make_uint4(pattern, pix, ((meta & 0xffffu) + 1u) | (((meta >> 16) - 1u) << 16),
                                sl | (n_prev_valid ? kPrevValid : 0u) | (n_delta ? kPrevDelta : 0u) | (n_med << kMediumShift)));
      if (n_lights) st_nt(&N.e[j], make_float4(hit_p.x, hit_p.y, hit_p.z, n_ppdf));
      if (P.has_motion) st_nt(&N.time[j], time);
    } else if (active) {
      st_nt(&staging[film_idx], make_float4(L.x, L.y, L.z, 0.0f));
    }
    const uint32_t q = seg0 + seg_append(want_shadow, &lds_ctr[1]);
    if (want_shadow) {
      st_nt(&Q.a[q], make_float4(hit_p.x, hit_p.y, hit_p.z, sh_tmax));
      st_nt(&Q.b[q], make_float4(sh_d.x, sh_d.y, sh_d.z, time));
      st_nt(&Q.c[q], make_float4(sh_c.x, sh_c.y, sh_c.z, __uint_as_float(alive ? j : (kFilmTarget | film_idx))));
      if (VOL)  // the vertex domain once more (tracer.rs:1121): the shadow segment's walk is seeded off it
        st_nt(&qseed[q], rng_seed(new_domain(new_domain(Sampler{pattern, P.sample_begin + sl}, (int)(meta & 0xffffu)), K_NEE_SHADOW)));
    }
    lap(5, false);
    __syncthreads();  // every lane has read its ring entry before CLASSIFY appends again
    lap(2, false);
    if (STAMPS) t_acc[6]++;
  }
  if (STAMPS && (threadIdx.x & 63) == 0)
    for (int s = 0; s < 8; s++) atomicAdd(s < 4 ? &C->cls_waves[s] : &C->cls_lanes[s - 4], t_acc[s]);
  add_stat(&lds_ctr[2], s_closest); add_stat(&lds_ctr[3], s_shadow); add_stat(&lds_ctr[4], s_vertices);
  add_stat(&lds_ctr[5], s_rr_t); add_stat(&lds_ctr[6], s_rr_k); add_stat(&lds_ctr[7], s_esc);
  add_stat(&lds_ctr[8], s_depth);
  __syncthreads();
  if (threadIdx.x == 0) {  // publish this segment's queues for the next stages (same workgroup index there)
    C->shadow[blockIdx.x] = lds_ctr[1];
  }
  if (threadIdx.x < kBins) {
    C->seg[1 - cur][blockIdx.x * kBins + threadIdx.x] = out_n[threadIdx.x];
    C->seg[cur][blockIdx.x * kBins + threadIdx.x] = 0;  // consumed: this buffer is the output of the next round
  }
  if (threadIdx.x >= 1 && threadIdx.x <= 7 && lds_ctr[threadIdx.x + 1])
    atomicAdd(&C->stats[threadIdx.x], (unsigned long long)lds_ctr[threadIdx.x + 1]);
}
template <int MATS, bool INF, bool WIDE, bool LIT, bool DRV>
__global__ __launch_bounds__(kBlock, WIDE ? CRT_SHADE_WIDE_WAVES : CRT_SHADE_WAVES) void k_shade(Params P, PathSoA S, PathSoA N, HitSoA H, ShadowSoA Q,
                                                                   Counters *C, int cur, float4 *staging, int first) {
  static_assert(LIT || !INF, "lights at infinity are lights");
  constexpr int ARENA = WIDE ? kArenaWide : kArenaDwords;
  __shared__ uint32_t sobol_tab[ARENA];
  shade_segment<MATS, INF ? 1 : 0, LIT, ARENA, DRV>(P, S, N, H, Q, C, cur, staging, sobol_tab, (first & 1) != 0, (first & 2) != 0);
}
// The instances of light lists that hold a mapped dome (CRT_LIGHT_DOME_MAP): k_shade<MATS, true, false, true, DRV> with
// the environment arm of light_sample_li_env / light_escaped_env compiled in. Kernels of their own, so that every other
// scene runs exactly the code it ran before mapped domes existed.
template <int MATS, bool DRV>
__global__ __launch_bounds__(kBlock, CRT_SHADE_WAVES) void k_shade_env(Params P, PathSoA S, PathSoA N, HitSoA H, ShadowSoA Q,
                                                                       Counters *C, int cur, float4 *staging, int first) {
  __shared__ uint32_t sobol_tab[kArenaDwords];
  shade_segment<MATS, 2, true, kArenaDwords, DRV>(P, S, N, H, Q, C, cur, staging, sobol_tab, (first & 1) != 0, (first & 2) != 0);
}

// The instances of volume renders: three waves, raw material records. INF as shade_segment's: 0 / 1 / 2 (mapped domes).
template <int MATS, int INF, bool LIT>
__global__ __launch_bounds__(kBlock, CRT_SHADE_WAVES) void k_shade_vol(Params P, PathSoA S, PathSoA N, HitSoA H, ShadowSoA Q,
                                                                       Counters *C, int cur, float4 *staging, int first, uint32_t *qseed) {
  static_assert(LIT || !INF, "lights at infinity are lights");
  __shared__ uint32_t sobol_tab[kArenaDwords];
  shade_segment<MATS, INF, LIT, kArenaDwords, false, true>(P, S, N, H, Q, C, cur, staging, sobol_tab, (first & 1) != 0, (first & 2) != 0, qseed);
}

// The instances of textured renders (LaunchPlan::faces), instantiated as k_shade_vol's: three waves, raw material records.
template <int MATS, int INF, bool LIT>
__global__ __launch_bounds__(kBlock, CRT_SHADE_WAVES) void k_shade_faces(Params P, PathSoA S, PathSoA N, HitSoA H, ShadowSoA Q,
                                                                         Counters *C, int cur, float4 *staging, int first, FaceView F,
                                                                         const uint4 *fplane) {
  static_assert(LIT || !INF, "lights at infinity are lights");
  __shared__ uint32_t sobol_tab[kArenaDwords];
  shade_segment<MATS, INF, LIT, kArenaDwords, false, false, true>(P, S, N, H, Q, C, cur, staging, sobol_tab, (first & 1) != 0, (first & 2) != 0,
                                                                  nullptr, &F, fplane);
}

// The instances of guided renders (LaunchPlan::guided), instantiated as k_shade_vol's: three waves, raw material records.
// The field's view is an argument of its own: wave-uniform, scalar registers.
template <int MATS, int INF, bool LIT>
__global__ __launch_bounds__(kBlock, CRT_SHADE_WAVES) void k_shade_guided(Params P, PathSoA S, PathSoA N, HitSoA H, ShadowSoA Q,
                                                                          Counters *C, int cur, float4 *staging, int first, GuideView G) {
  static_assert(LIT || !INF, "lights at infinity are lights");
  __shared__ uint32_t sobol_tab[kArenaDwords];
  shade_segment<MATS, INF, LIT, kArenaDwords, false, false, false, true>(P, S, N, H, Q, C, cur, staging, sobol_tab, (first & 1) != 0,
                                                                         (first & 2) != 0, nullptr, nullptr, nullptr, &G);
}

// ---- volume: the regions a segment crosses (volume.hip.h), between extend and shade of a volume render ----
// One live path per lane; a lane's spans and lobe weights are LDS columns [region][thread], as in volume_seam.hip. The
// VOLUME-FORWARD form, per path, with v the vertex domain and seed = rng_seed(new_domain(v, K_VOLUME)):
//   no region has an active interval on the segment: nothing is touched
//   depth exhausted (previous vertex valid, surface hit):  beta *= transmittance(ray, 0.001, t_hit)
//   otherwise:  E = sample_interaction(ray, 0.001, min(t_surf, t_med));  L += beta * E.emitted;  beta *= E.weight
//     passthrough: beta and L go back to the state; shade's medium, escape and surface arms run on them unchanged
//     scatter: the phase vertex (tracer.rs:1192-1249) is finished HERE — direction and pdf (K_PHASE), volume_nee
//       (K_NEE; phase value unclamped, light_weight(light_pdf, phase_val)), roulette on the multiplied beta (K_RR) — and
//       written over the path: a = p | dir.x, b = dir.yz | beta.xy, c = beta.z | L, e = contribution | phase_pdf, the hit
//       record = shadow direction | tmax, the hit word = kVolScatter | survived | shadow << 1. Plane d keeps the vertex's
//       words: shade's tail advances them.
// A walk that runs into CRT_VOLUME_STEP_LIMIT is the all-zero event (weight 0, emitted 0): the path goes on with beta = 0.
// first: camera paths, whose plane c generate did not write — it is written here for every path, so shade reads it.
__global__ __launch_bounds__(kBlock) void k_volume(Params P, PathSoA S, HitSoA H, Counters *C, int cur, int first, VolArgs V) {
  __shared__ uint32_t sobol_tab[kSobolLdsWords];
  __shared__ float span_a[kVolMaxRegions][kBlock], span_b[kVolMaxRegions][kBlock], lobe_w[kVolMaxRegions][kBlock];
  __shared__ uint32_t lds_ctr[8];  // [1..5] statistics, at their RayStats indices
  __shared__ uint32_t pre[kBins + 1];
  bins_prefix(&C->seg[cur][blockIdx.x * kBins], pre);
  const uint32_t n = pre[kBins];
  if (n == 0) return;  // uniform per workgroup
  if (threadIdx.x < 8) lds_ctr[threadIdx.x] = 0;
  sobol_tables_init(sobol_tab);  // ends with a workgroup barrier
  float *sa = &span_a[0][threadIdx.x], *sb = &span_b[0][threadIdx.x], *lw = &lobe_w[0][threadIdx.x];
  const uint32_t n_lights = P.n_lights;
  uint32_t s_closest = 0, s_shadow = 0, s_vertices = 0, s_rr_t = 0, s_rr_k = 0;
  for (uint32_t k = threadIdx.x; k < n; k += kBlock) {
    const uint32_t i = bin_slot(k, pre, P.seg_cap);
    const float4 A = S.a[i], B = S.b[i];
    const uint4 D = S.d[i];
    float4 Cc = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    if (!first) Cc = S.c[i];
    const uint32_t hg = H.geom[i];
    const bool has_hit = hg != kInvalid;
    const V3 ro = v3(A.x, A.y, A.z), rd = v3(A.w, B.x, B.y);
    V3 beta = v3(B.z, B.w, Cc.x), L = v3(Cc.y, Cc.z, Cc.w);
    const uint32_t pattern = D.x, meta = D.z, aux = D.w;
    const uint32_t n_rec = meta & 0xffffu;
    const int remaining = (int)(meta >> 16);
    const bool prev_valid = (aux & kPrevValid) != 0;
    const float t_surf = has_hit ? H.h[i].x : CRT_INF;
    const Sampler vdom = new_domain(Sampler{pattern, P.sample_begin + (aux & 0xffffu)}, (int)n_rec);  // tracer.rs:1121
    const uint32_t seed = rng_seed(new_domain(vdom, K_VOLUME));
    bool touched = false;
    if (remaining <= 0) {  // tracer.rs:1123-1149: the last segment only attenuates what its surface emits
      if (prev_valid && has_hit) {
        const VolSpans Sp = vol_active_intervals(V.regions, V.n_regions, ro, rd, 0.001f, t_surf, sa, sb, kBlock);
        if (Sp.mask != 0u) {
          V3 tr;
          (void)vol_transmittance_spans(V.regions, V.n_regions, V.grid, ro, rd, Sp, seed, sa, sb, kBlock, tr);
          beta = beta * tr;
          touched = true;
        }
      }
    } else {
      // the carried medium's free-flight candidate bounds the segment (tracer.rs:1159-1165): a pure function of the
      // vertex domain, so shade recomputes the same value
      float t_med = CRT_INF;
      const uint32_t med_id = aux >> kMediumShift;
      if (med_id) {
        const DevMedium med = P.media_by_id[med_id - 1];
        if (med.present && med.scattering) t_med = -(log_det(draw_rnd1(new_domain(vdom, K_MEDIUM)))) / med.sigma_bar;
      }
      const float t_end = t_med < t_surf ? t_med : t_surf;  // t_surf.min(t_med)
      const VolSpans Sp = vol_active_intervals(V.regions, V.n_regions, ro, rd, 0.001f, t_end, sa, sb, kBlock);
      if (Sp.mask != 0u) {
        const VolEvent E = vol_sample_interaction_spans(V.regions, V.n_regions, V.grid, ro, rd, Sp, seed, sa, sb, lw, kBlock);
        L = L + beta * E.emitted;
        beta = beta * E.weight;
        touched = true;
        if (E.kind == CRT_VOLUME_SCATTER) {  // === the phase vertex (tracer.rs:1192-1249) ===
          s_closest++;  // this iteration's World::intersect (tracer.rs:1152): shade skips the vertex it is counted in
          const V3 wi = normalize(rd);
          float ps[4];
          draw_sample4(new_domain(vdom, K_PHASE), ps, sobol_tab);
          V3 dir;
          float phase_pdf;
          vol_phase_sample(V.regions, V.n_regions, E, lw, kBlock, rd, ps[0], ps[1], ps[2], dir, phase_pdf);
          // volume_nee (tracer.rs:1040-1076)
          bool want_shadow = false;
          V3 sh_d = splat(0.0f), sh_c = splat(0.0f);
          float sh_tmax = 0.0f;
          if (P.strategy != CRT_STRATEGY_BSDF && n_lights > 0) {
            float nee_s[4];
            draw_sample4(new_domain(vdom, K_NEE), nee_s, sobol_tab);
            uint32_t li = (uint32_t)(nee_s[0] * (float)n_lights);  // LightList::pick, light.rs:421-429
            if (li > n_lights - 1) li = n_lights - 1;
            LightSample ls;
            if (light_sample_li_env<2>(P.lights[li], P.envs, E.p, nee_s[1], nee_s[2], ls)) {
              s_shadow++;
              want_shadow = true;
              sh_d = ls.direction;
              sh_tmax = ls.distance - 0.001f;
              const float phase_val = vol_phase_pdf(V.regions, V.n_regions, E, lw, kBlock, dot(wi, ls.direction));
              const float light_pdf = rmax(ls.pdf / (float)n_lights, 1e-6f);
              const V3 c = ((ls.radiance * phase_val) * light_weight(P.strategy, light_pdf, phase_val)) / light_pdf;
              sh_c = beta * c;
            }
          }
          bool survived = true;
          if (n_rec >= (uint32_t)kRrStartBounce) {
            s_rr_t++;
            const float p_survive = rclamp(max_elem(beta), kRrMinProb, 1.0f);
            if (p_survive < 1.0f) {
              if (draw_rnd1(new_domain(vdom, K_RR)) >= p_survive) {
                survived = false;
                s_rr_k++;
              } else {
                beta = beta / p_survive;
              }
            }
          }
          s_vertices++;
          S.a[i] = make_float4(E.p.x, E.p.y, E.p.z, dir.x);
          S.b[i] = make_float4(dir.y, dir.z, beta.x, beta.y);
          if (n_lights) {
            S.e[i] = make_float4(sh_c.x, sh_c.y, sh_c.z, phase_pdf);
            H.h[i] = make_float4(sh_d.x, sh_d.y, sh_d.z, sh_tmax);
          }
          H.geom[i] = kVolScatter | (survived ? 1u : 0u) | (want_shadow ? 2u : 0u);
        } else {
          S.b[i] = make_float4(B.x, B.y, beta.x, beta.y);
        }
      }
    }
    if (remaining <= 0 && touched) S.b[i] = make_float4(B.x, B.y, beta.x, beta.y);
    if (touched || first) S.c[i] = make_float4(beta.z, L.x, L.y, L.z);
  }
  add_stat(&lds_ctr[1], s_closest); add_stat(&lds_ctr[2], s_shadow); add_stat(&lds_ctr[3], s_vertices);
  add_stat(&lds_ctr[4], s_rr_t); add_stat(&lds_ctr[5], s_rr_k);
  __syncthreads();
  if (threadIdx.x >= 1 && threadIdx.x <= 5 && lds_ctr[threadIdx.x])
    atomicAdd(&C->stats[threadIdx.x], (unsigned long long)lds_ctr[threadIdx.x]);
}

// ---- shadow, volume renders: every request's contribution times the transmittance of its segment, before k_shadow pays
// the unoccluded ones out (the product is the last operation on the contribution: DESIGN.md §2). One request per lane;
// occluded requests are walked too. ----
__global__ __launch_bounds__(kBlock) void k_shadow_volume(Params P, ShadowSoA Q, const uint32_t *qseed, Counters *C, VolArgs V) {
  __shared__ float span_a[kVolMaxRegions][kBlock], span_b[kVolMaxRegions][kBlock];
  const uint32_t n = ((const volatile uint32_t *)C->shadow)[blockIdx.x];
  const uint32_t seg0 = blockIdx.x * P.seg_cap;
  float *sa = &span_a[0][threadIdx.x], *sb = &span_b[0][threadIdx.x];
  for (uint32_t k = threadIdx.x; k < n; k += kBlock) {  // n <= seg_cap: shade appended them
    const uint32_t q = seg0 + k;
    const float4 A = Q.a[q], B = Q.b[q];
    const V3 ro = v3(A.x, A.y, A.z), rd = v3(B.x, B.y, B.z);
    const VolSpans Sp = vol_active_intervals(V.regions, V.n_regions, ro, rd, 0.001f, A.w, sa, sb, kBlock);
    if (Sp.mask == 0u) continue;
    V3 tr;
    (void)vol_transmittance_spans(V.regions, V.n_regions, V.grid, ro, rd, Sp, qseed[q], sa, sb, kBlock, tr);
    float4 Cc = Q.c[q];
    Cc.x = Cc.x * tr.x; Cc.y = Cc.y * tr.y; Cc.z = Cc.z * tr.z;
    Q.c[q] = Cc;
  }
}

// ---- shade, PIPELINED: the four-wave kernel of unlit simple-material scenes with one material class (cornellbox, the
// bench) reads each path's state ONCE, and the reads of the next step travel while the current one computes. ----
// shade_segment's iteration is a serial chain: CLASSIFY loads 68 bytes of every path and waits, two barriers, the vertex
// step loads 84 bytes of every hit path AGAIN and waits, computes, stores. Nothing of step i + 1 is in flight while step
// i computes, and the kernel has no registers left to hold it (121 of 128). Here
//   * CLASSIFY reads the hit word only (4 bytes per path, requested one round ahead) and sorts slot numbers into two
//     rings: hits and misses;
//   * a STEP takes 256 entries of one ring — a vertex step (hits) or a miss step (escaped paths: sky, or the depth limit) —
//     so both kinds run on full waves;
//   * as soon as a wave has read the state of its current step out of its private LDS block it picks the entries of the
//     NEXT step and requests their planes with global_load_lds_dwordx4: per-lane source address, no destination
//     register, the block is written lane-linear (64 lanes x 16 bytes per plane). The loads are waited for (vmcnt) at the
//     top of the next iteration, a whole vertex computation later.
// Inside that span nothing may wait on the vector-memory counter early: the material table and the Sobol tables are read
// through LDS pointers (ds_read, not FLAT loads, which count on vmcnt too), the barriers are raw s_barrier behind an
// lgkmcnt wait (__syncthreads would drain vmcnt), and the only ordinary load — the next round's hit words — is used
// after the wait at the top. Per-path arithmetic, film slots and counters are shade_segment's; only the order in which a
// workgroup takes its paths differs, which no output depends on (the class rings and the lanes rely on the same).
//
// LDS budget of the pipelined instance (kArenaWide dwords): Sobol tables | material table | two rings | staging blocks.
constexpr uint32_t kPipeRing = 2 * kBlock;             // entries per ring: < kBlock pending + one classify round
constexpr int kPipePlanes = 5;                         // a b c d h, 1 KB per wave each, + 256 B of hit words
constexpr int kPipeWaveDwords = kPipePlanes * 256 + 64;
constexpr int kPipeStageDwords = (kBlock / 64) * kPipeWaveDwords;
constexpr int kPipeRingDwords = 2 * (int)kPipeRing;
constexpr int kMatDwords = (int)(sizeof(CrtMaterial) / 4);
// The rule the host applies (launch_plan.h, shade_pipe_fits): the pipelined instance runs only where the WHOLE material table
// fits beside its staging blocks; every other scene keeps k_shade and its LDS-resident table. (A lit scene's plane e would
// add 4 KB of staging and a partitioned scene's four rings 4 KB of rings: neither leaves room for a table.)
constexpr int kPipeMatMax = (kArenaWide - kSobolLdsWords - kPipeRingDwords - kPipeStageDwords) / kMatDwords;
static_assert(kPipeMatMax >= 6 && kSobolLdsWords + kPipeMatMax * kMatDwords + kPipeRingDwords + kPipeStageDwords <= kArenaWide,
              "Sobol tables + material table + rings + staging blocks fit the four-wave arena");
static_assert((kArenaWide - kPipeStageDwords) % 4 == 0 && kPipeWaveDwords % 4 == 0, "staging planes are 16-byte aligned");
// The SLIM instances (k_shade_pipe<DRV, true>): a hit-ring entry is the slot number AND the hit word CLASSIFY already
// holds (a vertex step takes it from there: no 4-byte fetch of it again, no staging row for it), and a wave's block is
// four planes — a, b, c or d, h: the first bounce reads plane d and no plane c, every later one the slim plane c and no
// plane d, so the two share a place. The wider ring is paid for by that plane.
constexpr int kSlimWaveDwords = 4 * 256;
constexpr int kSlimStageDwords = (kBlock / 64) * kSlimWaveDwords;
constexpr int kSlimRingDwords = 3 * (int)kPipeRing;  // hits: two dwords per entry; misses: one
static_assert(kSobolLdsWords + kPipeMatMax * kMatDwords + kSlimRingDwords + kSlimStageDwords <= kArenaWide,
              "the slim layout holds the same material table (kPipeMatMax is the host's one rule for both)");
static_assert((kArenaWide - kSlimStageDwords) % 4 == 0 && (kArenaWide - kSlimStageDwords - kSlimRingDwords) % 2 == 0,
              "slim staging planes are 16-byte aligned, hit-ring entries 8-byte aligned");
constexpr bool kShadePipeBuild = kBins == 1 && !kRegenFirst && CRT_SHADE_WIDE_WAVES == 4;
#ifndef CRT_SHADE_PIPE_HIT_REGS
#define CRT_SHADE_PIPE_HIT_REGS 0  // 1: the hit record of a vertex step by register loads at the top of the step, not staged (A/B)
#endif

typedef __attribute__((address_space(3))) void lds_void;
__device__ __forceinline__ void lds_dma16(const void *src, uint32_t *lds_dst /* wave-uniform */) {
  __builtin_amdgcn_global_load_lds(src, (lds_void *)lds_dst, 16, 0, 0);
}
__device__ __forceinline__ void lds_dma4(const void *src, uint32_t *lds_dst /* wave-uniform */) {
  __builtin_amdgcn_global_load_lds(src, (lds_void *)lds_dst, 4, 0, 0);
}
// A workgroup barrier that orders LDS accesses only: loads into LDS that are in flight stay in flight.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// Stamps (CRT_SHADE_STAMPS): [0] waiting for the staged state, [1] classify rounds with their barriers, [2] picking and
// requesting the next step, [3] vertex steps, [4] miss steps, [5] iterations, [6] rounds.
// SLIM: the instance that reads the slim path state (PathSoA) at every bounce but the first — `it` is the bounce number
// — and writes it unless out_full (the next consumer of N is not this kernel: k_path's tail, k_shade, nothing).
template <bool DRV, bool SLIM>
__device__ __forceinline__ void shade_segment_pipe(const Params &P, const PathSoA &S, const PathSoA &N, const HitSoA &H,
                                                   Counters *C, int cur, float4 *staging, uint32_t *arena /* kArenaWide */,
                                                   bool first, uint32_t it, bool out_full, bool append) {
  constexpr bool STAMPS = CRT_SHADE_STAMPS != 0;
  __shared__ uint32_t lds_ctr[10];   // [2..8] statistics
  __shared__ uint32_t out_n;         // survivors
  __shared__ uint32_t ring_tail[2];  // entries ever appended: hits, misses
  const uint32_t n = uniform(((const volatile uint32_t *)C->seg[cur])[blockIdx.x]);
  // append (uniform; behind k_camera_vertex): the other buffer's segment already holds that kernel's survivors, counted in
  // its seg word — this launch's survivors go behind them
  if (n == 0) {  // nothing lives in this segment: publish empty outputs and leave
    if (threadIdx.x == 0) { if (!append) C->seg[1 - cur][blockIdx.x] = 0; C->shadow[blockIdx.x] = 0; }
    return;
  }
  if (threadIdx.x < 10) lds_ctr[threadIdx.x] = 0;
  if (threadIdx.x == 0) out_n = append ? ((const volatile uint32_t *)C->seg[1 - cur])[blockIdx.x] : 0u;
  if (threadIdx.x < 2) ring_tail[threadIdx.x] = 0;
  sobol_tables_init(arena);  // ends with a workgroup barrier
  // the material table, always in LDS here (kPipeMatMax) and read through an LDS pointer
  uint32_t *mat_lds = arena + kSobolLdsWords;
  {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(MatTable<DRV>::of(P));
    const uint32_t words = P.n_materials * (uint32_t)kMatDwords;
    for (uint32_t w = threadIdx.x; w < words; w += kBlock) mat_lds[w] = src[w];
  }
  const typename MatTable<DRV>::Rec *mats = reinterpret_cast<const typename MatTable<DRV>::Rec *>(mat_lds);
  constexpr int STAGE = SLIM ? kSlimStageDwords : kPipeStageDwords, WAVE = SLIM ? kSlimWaveDwords : kPipeWaveDwords;
  constexpr int RINGS = SLIM ? kSlimRingDwords : kPipeRingDwords;
  uint32_t *ring_h = arena + kArenaWide - STAGE - RINGS, *ring_m = ring_h + (SLIM ? 2 : 1) * kPipeRing;
  uint32_t *stg = arena + kArenaWide - STAGE + (threadIdx.x >> 6) * WAVE;  // this wave's block
  const uint32_t lane = threadIdx.x & 63;
  __syncthreads();
  const uint32_t seg0 = blockIdx.x * P.seg_cap;  // kBins == 1: slot of the k-th live path = seg0 + k
  const bool compact = CRT_CAM_COMPACT_BUILD && first && P.cam_compact;  // uniform: camera paths are plane a's 16 bytes
  const bool compact_d = compact && P.cam_compact == 2;                  // uniform: ... and plane d's (root cull: compacted survivors)
  uint32_t s_closest = 0, s_vertices = 0, s_rr_t = 0, s_rr_k = 0, s_esc = 0, s_depth = 0;
  unsigned long long t_acc[7] = {0, 0, 0, 0, 0, 0, 0}, t0 = 0;
  auto lap = [&](int slot) {
    if (STAMPS) { const unsigned long long t = __builtin_readcyclecounter(); t_acc[slot] += t - t0; t0 = t; }
  };
  uint32_t next_in = 0, head_h = 0, head_m = 0, tail_h = 0, tail_m = 0;  // uniform
  uint32_t hg_next = threadIdx.x < n ? H.geom[seg0 + threadIdx.x] : kInvalid;  // the hit words of the next classify round
  uint32_t kind = 0, take = 0, k_in = 0;  // the current step: 0 none yet, 1 vertex, 2 miss; its entries' states are on their way
  uint32_t head_in = 0;                   // SLIM: where the current vertex step's entries sit in the hit ring (uniform)
  if (STAMPS) t0 = __builtin_readcyclecounter();
  for (;;) {
    // ---- the current step's state: out of this wave's staging block, into registers ----
    float4 A = make_float4(0.0f, 0.0f, 0.0f, 0.0f), B = make_float4(0.0f, 0.0f, 1.0f, 1.0f), Cc = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    float4 hh = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint4 D = make_uint4(0u, 0u, 0u, 0u);
    uint32_t hg = kInvalid;
    if (SLIM && kind) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's loads into its own block have landed
      A = reinterpret_cast<const float4 *>(stg)[lane];
      if (!first) {  // the slim form: L is +0, the depth words follow from the bounce number
        B = reinterpret_cast<const float4 *>(stg + 256)[lane];
        const float4 X = reinterpret_cast<const float4 *>(stg + 512)[lane];
        const uint32_t px = __float_as_uint(X.z);
        Cc = make_float4(X.x, 0.0f, 0.0f, 0.0f);
        D = make_uint4(__float_as_uint(X.y), px & 0x7fffffffu, (it & 0xffffu) | (((P.max_depth - it) & 0xffffu) << 16),
                       __float_as_uint(X.w) | kPrevValid | ((px >> 31) ? kPrevDelta : 0u));
      } else if (!compact) {
        B = reinterpret_cast<const float4 *>(stg + 256)[lane];
        D = reinterpret_cast<const uint4 *>(stg + 512)[lane];
      } else if (compact_d) {
        D = reinterpret_cast<const uint4 *>(stg + 512)[lane];
      }
      if (kind == 1) {
        // the hit word from the ring entry: nothing appends between a step's pick and this read (the next CLASSIFY
        // round starts behind a barrier every wave reaches after it)
        hh = CRT_SHADE_PIPE_HIT_REGS ? H.h[seg0 + k_in] : reinterpret_cast<const float4 *>(stg + 768)[lane];
        hg = ring_h[2 * ((head_in + threadIdx.x) % kPipeRing) + 1];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // ... and are in registers: the block may be overwritten
    } else if (kind) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's loads into its own block have landed
      A = reinterpret_cast<const float4 *>(stg)[lane];
      if (!compact) {
        B = reinterpret_cast<const float4 *>(stg + 256)[lane];
        D = reinterpret_cast<const uint4 *>(stg + 768)[lane];
        if (!first) Cc = reinterpret_cast<const float4 *>(stg + 512)[lane];
      } else if (compact_d) {
        D = reinterpret_cast<const uint4 *>(stg + 768)[lane];
      }
      if (kind == 1 && CRT_SHADE_PIPE_HIT_REGS) {
        hh = H.h[seg0 + k_in];
        hg = H.geom[seg0 + k_in];
      } else if (kind == 1) {
        hh = reinterpret_cast<const float4 *>(stg + 1024)[lane];
        hg = stg[1280 + lane];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // ... and are in registers: the block may be overwritten
    }
    lap(0);
    // ---- CLASSIFY rounds while both rings have room for one and input remains ----
    while (next_in < n && tail_h - head_h < (uint32_t)kBlock && tail_m - head_m < (uint32_t)kBlock) {
      lds_barrier();  // every wave has read the ring entries and the tails of the round before
      const uint32_t k_c = next_in + threadIdx.x;
      const uint32_t hg_c = hg_next;
      next_in += kBlock;
      hg_next = kInvalid;
      if (next_in + threadIdx.x < n) hg_next = H.geom[seg0 + next_in + threadIdx.x];
      const bool hit = k_c < n && hg_c != kInvalid, miss = k_c < n && hg_c == kInvalid;
      const uint32_t at_h = seg_append(hit, &ring_tail[0]);
      if (SLIM) { if (hit) reinterpret_cast<uint2 *>(ring_h)[at_h % kPipeRing] = make_uint2(k_c, hg_c); }
      else if (hit) ring_h[at_h % kPipeRing] = k_c;
      const uint32_t at_m = seg_append(miss, &ring_tail[1]);
      if (miss) ring_m[at_m % kPipeRing] = k_c;
      lds_barrier();
      tail_h = uniform(ring_tail[0]);
      tail_m = uniform(ring_tail[1]);
      if (STAMPS) t_acc[6]++;
    }
    lap(1);
    // ---- the next step: a workgroup's worth of hits, else of misses, else (input exhausted) what is left ----
    const uint32_t pend_h = tail_h - head_h, pend_m = tail_m - head_m;
    uint32_t kind_n = 0, take_n = 0, k_n = 0;
    if (pend_h >= (uint32_t)kBlock || (pend_h && pend_m < (uint32_t)kBlock)) { kind_n = 1; take_n = pend_h < (uint32_t)kBlock ? pend_h : (uint32_t)kBlock; }
    else if (pend_m) { kind_n = 2; take_n = pend_m < (uint32_t)kBlock ? pend_m : (uint32_t)kBlock; }
    const uint32_t head_n = head_h;
    if (SLIM && kind_n && threadIdx.x < take_n) {
      k_n = kind_n == 1 ? ring_h[2 * ((head_h + threadIdx.x) % kPipeRing)] : ring_m[(head_m + threadIdx.x) % kPipeRing];
      const uint32_t i_n = seg0 + k_n;
      lds_dma16(&S.a[i_n], stg);
      if (!first) {
        lds_dma16(&S.b[i_n], stg + 256);
        lds_dma16(&S.c[i_n], stg + 512);
      } else if (!compact) {
        lds_dma16(&S.b[i_n], stg + 256);
        lds_dma16(&S.d[i_n], stg + 512);
      } else if (compact_d) {
        lds_dma16(&S.d[i_n], stg + 512);
      }
      if (kind_n == 1 && !CRT_SHADE_PIPE_HIT_REGS) lds_dma16(&H.h[i_n], stg + 768);
    } else if (kind_n && threadIdx.x < take_n) {
      k_n = kind_n == 1 ? ring_h[(head_h + threadIdx.x) % kPipeRing] : ring_m[(head_m + threadIdx.x) % kPipeRing];
      const uint32_t i_n = seg0 + k_n;
      lds_dma16(&S.a[i_n], stg);
      if (!compact) {
        lds_dma16(&S.b[i_n], stg + 256);
        lds_dma16(&S.d[i_n], stg + 768);
        if (!first) lds_dma16(&S.c[i_n], stg + 512);
      } else if (compact_d) {
        lds_dma16(&S.d[i_n], stg + 768);
      }
      if (kind_n == 1 && !CRT_SHADE_PIPE_HIT_REGS) {
        lds_dma16(&H.h[i_n], stg + 1024);
        lds_dma4(&H.geom[i_n], stg + 1280);
      }
    }
    head_h += kind_n == 1 ? take_n : 0u;
    head_m += kind_n == 2 ? take_n : 0u;
    lap(2);
    const bool active = threadIdx.x < take;
    if (kind == 2) {
      // ---- MISS step (tracer.rs:1321-1342, :1123-1149): the path ends on the sky gradient, or at the depth limit ----
      if (active) {
        if (compact) compact_camera_path<true>(P, k_in, A, A, B, D);
        const int remaining = (int)(D.z >> 16);
        const V3 rd = v3(A.w, B.x, B.y), beta = v3(B.z, B.w, Cc.x);
        V3 L = v3(Cc.y, Cc.z, Cc.w);
        if (remaining > 0) {
          s_closest++;
          s_esc++;
          L = escaped_to_sky(rd, beta, L);
        } else {  // depth exhausted: nothing is added
          s_depth++;
          if ((D.w & kPrevValid) != 0) s_closest++;
        }
        st_nt(&staging[(D.w & 0xffffu) * P.n_act + D.y], make_float4(L.x, L.y, L.z, 0.0f));
      }
      lap(4);
    } else if (kind == 1) {
      // ---- VERTEX step: shade_segment's, for a hit on a simple material in a scene without lights or media ----
      bool alive = false;
      V3 L = splat(0.0f), beta = splat(1.0f), n_o = splat(0.0f), n_d = splat(0.0f);
      uint32_t meta = 0, aux = 0, pix = 0, pattern = 0;
      bool n_delta = false;
      if (active) {
        if (compact) compact_camera_path<true>(P, k_in, A, A, B, D);
        const V3 ro = v3(A.x, A.y, A.z), rd = v3(A.w, B.x, B.y);
        beta = v3(B.z, B.w, Cc.x);
        L = v3(Cc.y, Cc.z, Cc.w);
        pattern = D.x; pix = D.y; meta = D.z; aux = D.w;
        const uint32_t n_rec = meta & 0xffffu;
        const int remaining = (int)(meta >> 16);
        const bool prev_valid = (aux & kPrevValid) != 0;
        const uint32_t mat_i = hg & 0x7fffffffu;  // the material record's index: the geometry id
        HitRec rec;
        rec.front_face = ((hg >> 31) & 1u) != 0;
        rec.t = hh.x;
        rec.normal = v3(hh.y, hh.z, hh.w);
        rec.p = ro + rd * rec.t;  // ray.at(t), rt_world.rs:221
        const auto mat = MatTable<DRV>::view(mats, P, mat_i);
        // the vertex itself: vertex_simple.hip.h, the one source this kernel shares with k_camera_vertex
        const VertexOut v = vertex_simple(mat, ro, rd, beta, L, rec, pattern, P.sample_begin + (aux & 0xffffu), n_rec, remaining,
                                          prev_valid, arena);
        beta = v.beta; L = v.L;
        alive = v.alive;
        n_o = v.origin; n_d = v.dir; n_delta = v.delta;  // zero / false where the path ended
        s_closest += v.closest; s_vertices += v.vertices; s_rr_t += v.rr_tested; s_rr_k += v.rr_killed; s_esc += v.escaped;
        s_depth += v.depth_ended;
      }
      // survivors go to the other state buffer, finished paths to the film
      const uint32_t j = seg0 + seg_append(alive, &out_n);
      const uint32_t sl = aux & 0xffffu;
      if (alive) {
        st_nt(&N.a[j], make_float4(n_o.x, n_o.y, n_o.z, n_d.x));
        st_nt(&N.b[j], make_float4(n_d.y, n_d.z, beta.x, beta.y));
        if (SLIM && !out_full) {  // uniform: the next launch on this buffer is this kernel again
          st_nt(&N.c[j], make_float4(beta.z, __uint_as_float(pattern), __uint_as_float(pix | (n_delta ? 0x80000000u : 0u)), __uint_as_float(sl)));
        } else {
          st_nt(&N.c[j], make_float4(beta.z, L.x, L.y, L.z));
          st_nt(&N.d[j], make_uint4(pattern, pix, ((meta & 0xffffu) + 1u) | (((meta >> 16) - 1u) << 16),
                                    sl | kPrevValid | (n_delta ? kPrevDelta : 0u)));
        }
      } else if (active) {
        st_nt(&staging[sl * P.n_act + pix], make_float4(L.x, L.y, L.z, 0.0f));
      }
      lap(3);
    }
    if (STAMPS) t_acc[5]++;
    if (!kind_n) break;  // uniform: input exhausted and nothing pending
    kind = kind_n; take = take_n; k_in = k_n; head_in = head_n;
  }
  add_stat(&lds_ctr[2], s_closest); add_stat(&lds_ctr[4], s_vertices);
  add_stat(&lds_ctr[5], s_rr_t); add_stat(&lds_ctr[6], s_rr_k); add_stat(&lds_ctr[7], s_esc);
  add_stat(&lds_ctr[8], s_depth);
  __syncthreads();
  if (threadIdx.x == 0) {  // publish this segment's queues for the next stages (same workgroup index there)
    C->shadow[blockIdx.x] = 0;
    C->seg[1 - cur][blockIdx.x] = out_n;
    C->seg[cur][blockIdx.x] = 0;  // consumed: this buffer is the output of the next round
  }
  if (threadIdx.x >= 1 && threadIdx.x <= 7 && lds_ctr[threadIdx.x + 1])
    atomicAdd(&C->stats[threadIdx.x], (unsigned long long)lds_ctr[threadIdx.x + 1]);
  if (STAMPS && lane == 0)
    for (int s = 0; s < 7; s++) atomicAdd(s < 4 ? &C->cls_waves[s] : &C->cls_lanes[s - 4], t_acc[s]);
}
// it, out_full: read by the SLIM instances only. first: bit 0 the camera paths' launch, bit 1 append (shade_segment_pipe).
template <bool DRV, bool SLIM = false>
__global__ __launch_bounds__(kBlock, CRT_SHADE_WIDE_WAVES) void k_shade_pipe(Params P, PathSoA S, PathSoA N, HitSoA H, Counters *C,
                                                                              int cur, float4 *staging, int first, uint32_t it,
                                                                              int out_full) {
  __shared__ __attribute__((aligned(16))) uint32_t arena[kArenaWide];
  shade_segment_pipe<DRV, SLIM>(P, S, N, H, C, cur, staging, arena, (first & 1) != 0, it, out_full != 0, (first & 2) != 0);
}

// ---- camera + first vertex: k_camera with the first shade's vertex step behind the trace (LaunchPlan::camera_vertex) ----
// At bounce 0 nearly every live path is a hit, and k_camera holds its ray, t and primitive in registers — yet it wrote
// planes a, d and the hit record (52 bytes per path) for a first k_shade_pipe launch that sorts slots none of which
// needs sorting and gathers the same 52 bytes back through its staging blocks. Here the lane that traced the ray shades
// its first vertex (vertex_simple.hip.h, the function k_shade_pipe's vertex step calls) with a camera path's constants as
// literals — origin = the camera's, throughput 1, radiance 0, no vertex recorded, no previous vertex — so the roulette
// and previous-vertex arms fold away and the arithmetic left is the first shade's, operation for operation.
//   CAM_HIT    the vertex; a survivor goes to the OTHER state buffer N, compacted with an LDS counter, in the form the
//              next launch reads (slim_out: planes a, b and the slim c; otherwise the full four planes), a finished path
//              to its staging film slot
//   CAM_MISS   finished here as the cull arm finishes its rays: the miss step's arithmetic and counters
//   CAM_DEFER  the ray goes to the input buffer S, compacted with a second LDS counter, in the root-cull compact form
//              (planes a and d, Params::cam_compact == 2 — the caller launches the first extend and shade with that
//              value whatever the cull says): the ordinary extend instance traces the segment's seg[0] rays, the first
//              k_shade_pipe launch shades them in append mode behind the survivors counted in seg[1]
// The eight RayStats totals keep their values: closest_hit and vertices per hit, closest_hit and escaped per miss, as the
// first shade would have added them. LDS: the material table (at most kPipeMatMax records, as k_shade_pipe stages it)
// beside k_camera's Sobol tables, node window and stacks — the window keeps its kCamWindow strides.
static_assert((kSobolLdsWords + kCamLdsDwords + kPipeMatMax * kMatDwords) * 4 + 512 <= 40 * 1024, "four workgroups of k_camera_vertex per CU");
// TABLE, ROOT_LDS: as k_camera's — the per-pixel table and the sample cursor in the sample loop; the cull's root from LDS.
template <bool DRV, bool TABLE, bool ROOT_LDS>
__global__ __launch_bounds__(kBlock, 4) void k_camera_vertex(Params P, PathSoA S, PathSoA N, Counters *C, uint32_t sample_begin,
                                                             uint32_t n_samples, float4 *staging, uint32_t mode, int slim_out,
                                                             const PixelRec *pixel_table) {
  __shared__ uint32_t sobol_tab[kSobolLdsWords];
  __shared__ __attribute__((aligned(16))) uint32_t cam_lds[kCamLdsDwords];
  __shared__ __attribute__((aligned(16))) uint32_t mat_lds[kPipeMatMax * kMatDwords];
  __shared__ uint32_t cam_ctr[4];  // rays left to the first extend | camera rays that escaped here | survivors | vertices
  const bool cull = P.root_cull != 0;  // uniform
  float bmin[3][4] = {}, bmax[3][4] = {};
  uint32_t child[4] = {};
  if (!ROOT_LDS) {
    const WideNode &root = P.scene.nodes[P.scene.root];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int l = 0; l < 4; l++) { bmin[a][l] = root.bmin[a][l]; bmax[a][l] = root.bmax[a][l]; }
#pragma unroll
    for (int l = 0; l < 4; l++) child[l] = root.child[l];
  }
  if (threadIdx.x < 4) cam_ctr[threadIdx.x] = 0;
  {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(MatTable<DRV>::of(P));
    // at most kPipeMatMax records (plan_launches, shade_pipe_fits)
    const uint32_t words = (P.n_materials < (uint32_t)kPipeMatMax ? P.n_materials : (uint32_t)kPipeMatMax) * (uint32_t)kMatDwords;
    for (uint32_t w = threadIdx.x; w < words; w += kBlock) mat_lds[w] = src[w];
  }
  const typename MatTable<DRV>::Rec *mats = reinterpret_cast<const typename MatTable<DRV>::Rec *>(mat_lds);
  uint32_t *lds_nodes = cam_lds;
  uint32_t *stk = cam_lds + kCamWindow * kLdsNodeStride + threadIdx.x;  // entry e of this lane: stk[e * kBlock]
  uint32_t n_lds_pk;
  const uint32_t n_lds = stage_nodes(P.scene, lds_nodes, kCamWindow, n_lds_pk);  // ends with a workgroup barrier
  sobol_tables_init(sobol_tab);                                                  // ... as does this
  const bool defer_all = (mode & 1u) != 0;
  const uint32_t want_stack = mode >> 8;
  const uint32_t pstack = (want_stack == 0 || want_stack > (uint32_t)kCamStack) ? (uint32_t)kCamStack : want_stack;
  const size_t total = (size_t)P.n_act * n_samples;
  const size_t seg0 = (size_t)blockIdx.x * kBins * P.seg_cap;
  const V3 cam_o = ld3(P.camera.origin) + splat(0.0f);  // the pinhole camera's origin, as the compact form's readers take it
  uint32_t n_escaped = 0, n_vertices = 0;
  // TABLE: this lane's pixel slot and sample, round by round, and the pixel's record, loaded a round ahead
  SampleCursor at_g = {0, 0, 0, 0};
  uint4 rec0 = make_uint4(0, 0, 0, 0), rec1 = make_uint4(0, 0, 0, 0);
  if (TABLE) {
    at_g = sample_cursor(camera_slot_sample(threadIdx.x), (unsigned long long)gridDim.x * kBlock, P.n_act);
    pixel_rec_load(P, pixel_table, at_g.pix, rec0, rec1);
  }
  for (size_t k0 = 0; k0 < P.seg_cap; k0 += kBlock) {  // uniform: seg_cap is a multiple of the workgroup's width
    if (camera_slot_sample(k0) >= total) break;        // uniform
    const size_t g = camera_slot_sample(k0 + threadIdx.x);
    const uint32_t t_pix = at_g.pix, t_sl = at_g.sl;
    const uint4 t_rec0 = rec0, t_rec1 = rec1;
    if (TABLE) {  // the next round's record: its slot is below n_act whether or not that round exists
      sample_cursor_next(at_g, P.n_act);
      pixel_rec_load(P, pixel_table, at_g.pix, rec0, rec1);
    }
    CameraSample cs;
    cs.o = splat(0.0f); cs.d = splat(0.0f); cs.time = 0.0f; cs.pattern = 0; cs.pix = 0; cs.sl = 0;
    int res = CAM_MISS;
    bool valid = false, alive = false;
    VertexOut v;
    v.origin = splat(0.0f); v.dir = splat(0.0f); v.beta = splat(1.0f); v.L = splat(0.0f); v.delta = false;
    if (g < total) {
      if (TABLE) cs = camera_sample_table(P, t_rec0, t_rec1, t_pix, t_sl, sample_begin, sobol_tab);
      else cs = camera_sample(P, g, sample_begin, sobol_tab);
      valid = true;
      bool keep = true;
      if (cull)  // uniform
        keep = ROOT_LDS ? root_touched_lds(lds_nodes + (size_t)P.scene.root * kLdsNodeStride, cs.o, cs.d)
                        : node_touched(bmin, bmax, child, cs.o.x, cs.o.y, cs.o.z, cs.d.x, cs.d.y, cs.d.z, 0.001f, CRT_INF);
      float t = 0.0f;
      uint32_t prim = kInvalid;
      if (keep)
        res = defer_all ? (int)CAM_DEFER
                        : camera_trace(P.scene, lds_nodes, n_lds, n_lds_pk, stk, kBlock, pstack, 0.001f, CRT_INF, CRT_MASK_CAMERA,
                                       cam_o.x, cam_o.y, cam_o.z, cs.d.x, cs.d.y, cs.d.z, t, prim);
      const uint32_t sl = cs.sl & 0xffffu;
      if (res == CAM_HIT) {  // the first shade's VERTEX step on a camera path
        float4 h;
        uint32_t gw;
        camera_hit_record(P.scene, prim, t, cs.d.x, cs.d.y, cs.d.z, h, gw);
        HitRec rec;
        rec.front_face = ((gw >> 31) & 1u) != 0;
        rec.t = h.x;
        rec.normal = v3(h.y, h.z, h.w);
        rec.p = cam_o + cs.d * rec.t;  // ray.at(t), rt_world.rs:221
        const auto mat = MatTable<DRV>::view(mats, P, gw & 0x7fffffffu);
        v = vertex_simple(mat, cam_o, cs.d, splat(1.0f), splat(0.0f), rec, cs.pattern, P.sample_begin + sl, 0u, (int)P.max_depth, false,
                          sobol_tab);
        alive = v.alive;
        n_vertices++;
        if (!alive) st_nt(&staging[sl * P.n_act + cs.pix], make_float4(v.L.x, v.L.y, v.L.z, 0.0f));
      } else if (res == CAM_MISS) {  // tracer.rs:1321-1342 with L = 0, beta = 1: the first shade's miss step (the cull arm's too)
        const V3 L = escaped_to_sky(cs.d, splat(1.0f), splat(0.0f));
        st_nt(&staging[sl * P.n_act + cs.pix], make_float4(L.x, L.y, L.z, 0.0f));
        n_escaped++;
      }
    }
    // survivors to the other buffer, deferred rays to this one: every wave appends in every round
    const size_t j = seg0 + seg_append(alive, &cam_ctr[2]);
    if (alive) {
      const uint32_t sl = cs.sl & 0xffffu;
      st_nt(&N.a[j], make_float4(v.origin.x, v.origin.y, v.origin.z, v.dir.x));
      st_nt(&N.b[j], make_float4(v.dir.y, v.dir.z, v.beta.x, v.beta.y));
      if (slim_out) {  // uniform: the next shade launch is the slim instance
        st_nt(&N.c[j], make_float4(v.beta.z, __uint_as_float(cs.pattern), __uint_as_float(cs.pix | (v.delta ? 0x80000000u : 0u)), __uint_as_float(sl)));
      } else {
        st_nt(&N.c[j], make_float4(v.beta.z, v.L.x, v.L.y, v.L.z));
        st_nt(&N.d[j], make_uint4(cs.pattern, cs.pix, 1u | (((P.max_depth & 0xffffu) - 1u) << 16), sl | kPrevValid | (v.delta ? kPrevDelta : 0u)));
      }
    }
    const bool later = valid && res == CAM_DEFER;
    const size_t i = seg0 + seg_append(later, &cam_ctr[0]);
    if (later) {
      st_nt(&S.a[i], make_float4(cs.d.x, cs.d.y, cs.d.z, __uint_as_float(cs.pattern)));
      st_nt(&S.d[i], make_uint4(cs.pattern, cs.pix, (P.max_depth & 0xffffu) << 16, cs.sl));
    }
  }
  add_stat(&cam_ctr[1], n_escaped);
  add_stat(&cam_ctr[3], n_vertices);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int b = 0; b < kBins; b++) {
      C->seg[0][blockIdx.x * kBins + b] = b == 0 ? cam_ctr[0] : 0;
      C->seg[1][blockIdx.x * kBins + b] = b == 0 ? cam_ctr[2] : 0;
    }
    C->shadow[blockIdx.x] = 0;
    C->cam_defer[blockIdx.x] = 0;
    if (blockIdx.x == 0) atomicAdd(&C->stats[0], (unsigned long long)total);  // camera_rays (tracer.rs:585)
    // what the first shade would have added: closest_hit and vertices per hit; closest_hit and escaped per miss
    const uint32_t esc = cam_ctr[1], hit = cam_ctr[3];
    if (esc + hit) atomicAdd(&C->stats[1], (unsigned long long)(esc + hit));
    if (hit) atomicAdd(&C->stats[3], (unsigned long long)hit);
    if (esc) atomicAdd(&C->stats[6], (unsigned long long)esc);
  }
}

// ---- shadow: World::occluded (rt_world.rs:235-237) for the queue; unoccluded requests pay out ----
// CURVE: kColdCurve in the instances that run curve images (the any-hit engine keeps no other cold state apart)
template <bool STATS, int WIDE, int CURVE = 0>
__device__ __forceinline__ void shadow_segment(const Params &P, const PathSoA &N, const ShadowSoA &Q, Counters *C,
                                               float4 *staging, CrtTravStats *tstats, uint32_t *engine_lds) {
  const uint32_t n = ((const volatile uint32_t *)C->shadow)[blockIdx.x];
  if (n == 0) return;  // uniform per workgroup
  __shared__ uint32_t next;
  if (threadIdx.x == 0) next = 0;
  const uint32_t seg0 = blockIdx.x * P.seg_cap;
  LaneStats st = {};
  uint32_t err = 0, done = 0;
  auto fetch = [&](bool want, RayIn &in) -> bool {
    uint32_t k;
    if (!lds_take(want, &next, n, k)) return false;
    const uint32_t q = seg0 + k;
    const float4 A = Q.a[q], B = Q.b[q];
    in.ox = A.x; in.oy = A.y; in.oz = A.z; in.dx = B.x; in.dy = B.y; in.dz = B.z;
    in.time = B.w; in.mask = CRT_MASK_SHADOW; in.t_min = 0.001f; in.t_max = A.w; in.slot = q;
    return true;
  };
  auto emit = [&](uint32_t q, bool occ, const Hit &, float, float, float) {
    done++;
    if (occ) return;
    const float4 Cc = Q.c[q];
    const uint32_t tg = __float_as_uint(Cc.w);
    if (tg & kFilmTarget) {  // the path ended at this vertex: its radiance already sits in the staging plane
      const uint32_t f = tg & ~kFilmTarget;
      float4 v = staging[f];
      v.x = v.x + Cc.x; v.y = v.y + Cc.y; v.z = v.z + Cc.z;
      staging[f] = v;
    } else {  // beta.z | L.xyz
      float4 v = N.c[tg];
      v.y = v.y + Cc.x; v.z = v.z + Cc.y; v.w = v.w + Cc.z;
      N.c[tg] = v;
    }
  };
  run_traversal<true, STATS, WIDE, (int)kColdAll | CURVE, WIDE != 0>(P.scene, engine_lds, 0.001f, err, st, fetch, emit, CRT_MASK_SHADOW);
  if (err) atomicOr(&C->err, err);
  if (STATS) flush_stats(st, tstats, done);
}
template <bool STATS, int WIDE>
__global__ __launch_bounds__(kBlock, WIDE ? 4 : CRT_SHADOW_WAVES) void k_shadow(Params P, PathSoA N, ShadowSoA Q, Counters *C,
                                                                     float4 *staging, CrtTravStats *tstats) {
  __shared__ __attribute__((aligned(16))) uint32_t engine_lds[WIDE ? kEngineLdsWide : kEngineLdsDwords];
  shadow_segment<STATS, WIDE>(P, N, Q, C, staging, tstats, engine_lds);
}
// the three-wave instance with the rounded-cone arm: images that hold curve segments (DevScene::cold, kColdCurve)
template <bool STATS>
__global__ __launch_bounds__(kBlock, CRT_SHADOW_WAVES) void k_shadow_curve(Params P, PathSoA N, ShadowSoA Q, Counters *C,
                                                                        float4 *staging, CrtTravStats *tstats) {
  __shared__ __attribute__((aligned(16))) uint32_t engine_lds[kEngineLdsDwords];
  shadow_segment<STATS, 0, (int)kColdCurve>(P, N, Q, C, staging, tstats, engine_lds);
}
// ... and with the cubic span's walk beside it: images that hold cubic spans (kColdCubic)
template <bool STATS>
__global__ __launch_bounds__(kBlock, CRT_SHADOW_WAVES) void k_shadow_cubic(Params P, PathSoA N, ShadowSoA Q, Counters *C,
                                                                        float4 *staging, CrtTravStats *tstats) {
  __shared__ __attribute__((aligned(16))) uint32_t engine_lds[kEngineLdsDwords];
  shadow_segment<STATS, 0, (int)(kColdCurve | kColdCubic)>(P, N, Q, C, staging, tstats, engine_lds);
}

// ---- the whole path loop of one wavefront batch in ONE launch. Queue segments are private to their workgroup at
// every stage (generate, extend, shade and shadow of segment b all run in workgroup b), so nothing but a workgroup
// barrier separates the stages: no grid-wide barrier, no launch per bounce, and workgroups drift apart freely — while
// one is shading (VALU-bound) its neighbours on the same SIMDs are traversing (latency-bound). A workgroup leaves as
// soon as its segment is empty. LIT: the scene has lights and the strategy samples them (shadow stage present). ----
// No instance for lights at infinity: those scenes (outside SURVEY §8) always run the per-stage launches. The one fault
// this code base ever showed — round 2, run-to-run differences of a few ulps — was confined to k_path<., LIT, INF> of
// one build, whose per-stage launches of the same shade code were exact; its cause was never established
// (profiles/README.md, "The round-2 nondeterminism"), so that kernel family is not built.
template <int MATS, bool LIT, int COLD, bool DRV>
__global__ __launch_bounds__(kBlock, CRT_EXTEND_WAVES) void k_path(Params P, PathSoA S0, PathSoA S1, HitSoA H, ShadowSoA Q, Counters *C,
                                                 float4 *staging, uint32_t sample_begin, uint32_t n_samples,
                                                 uint32_t start_it, int cur0) {
  __shared__ __attribute__((aligned(16))) uint32_t arena[kArenaDwords];
  __shared__ uint32_t live;
  // start_it > 0: the TAIL of a per-stage batch — the paths still alive after `start_it` bounces sit in buffer `cur0`
  // of their segments (written by the last k_shade launch); this launch runs what is left of the path loop
  if (start_it == 0) {
    generate_segment(P, S0, C, sample_begin, n_samples, arena, true);
    __syncthreads();
  }
  int cur = cur0;
  for (uint32_t it = start_it; it <= P.max_depth; it++) {
    const PathSoA &S = cur ? S1 : S0;
    const PathSoA &N = cur ? S0 : S1;
    extend_segment<false, false, COLD, false>(P, S, H, C, cur, it == 0 ? 1 : 0, nullptr, arena);
    __syncthreads();  // hit records of this segment are complete; the arena changes hands
    shade_segment<MATS, false, LIT, kArenaDwords, DRV>(P, S, N, H, Q, C, cur, staging, arena, false);
    __syncthreads();
    if (LIT) {
      shadow_segment<false, false, COLD & (int)(kColdCurve | kColdCubic)>(P, N, Q, C, staging, nullptr, arena);
      __syncthreads();
    }
    cur = 1 - cur;
    if (threadIdx.x == 0) {
      uint32_t n = 0;
      for (int b = 0; b < kBins; b++) n += ((const volatile uint32_t *)C->seg[cur])[blockIdx.x * kBins + b];
      live = n;
    }
    __syncthreads();
    if (live == 0) break;  // uniform: every path of this segment has ended
  }
}

// ---- resolve: sum += color, in sample order; weight_sum += wx*wy = 1 (tracer.rs:599-600) ----
__global__ __launch_bounds__(kBlock) void k_resolve(const float4 *staging, uint32_t n_pix, uint32_t n_samples,
                                                    float4 *film /* r, g, b sums and weight_sum */) {
  for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < n_pix; p += gridDim.x * kBlock) {
    float4 acc = film[p];
    for (uint32_t s = 0; s < n_samples; s++) {
      const float4 v = staging[(size_t)s * n_pix + p];
      acc.x = acc.x + v.x; acc.y = acc.y + v.y; acc.z = acc.z + v.z;
      acc.w = acc.w + 1.0f;
    }
    film[p] = acc;
  }
}

// ---- adaptive variant (tracer.rs:599-617): the same fold, plus the luminance statistics in f64 and the stopping
// rule evaluated after every 4th sample once min_spp are in — exactly where render_pixel evaluates it. A pixel that
// stops ignores the rest of the batch (those samples were traced but are not part of its estimate). ----
__global__ __launch_bounds__(kBlock) void k_resolve_adaptive(const float4 *staging, const uint32_t *active, uint32_t n_act,
                                                             uint32_t n_samples, float4 *film, PixelStats *stats,
                                                             uint32_t *state /* taken | stopped << 31 */,
                                                             uint32_t min_spp, float variance_threshold) {
  const double threshold = (double)variance_threshold;
  for (uint32_t a = blockIdx.x * kBlock + threadIdx.x; a < n_act; a += gridDim.x * kBlock) {
    const uint32_t p = active ? active[a] : a;
    float4 acc = film[p];
    PixelStats ps = stats[p];
    uint32_t st = state[p];
    uint32_t taken = st & 0x7fffffffu;
    bool stopped = (st >> 31) != 0;
    for (uint32_t s = 0; s < n_samples && !stopped; s++) {
      const float4 v = staging[(size_t)s * n_act + a];
      acc.x = acc.x + v.x; acc.y = acc.y + v.y; acc.z = acc.z + v.z;
      acc.w = acc.w + 1.0f;
      const double lum = (double)(0.2126f * v.x + 0.7152f * v.y + 0.0722f * v.z);  // guiding/mod.rs:18-20
      ps.lum_sum += lum;
      ps.lum_sq += lum * lum;
      taken++;
      if (threshold > 0.0 && taken >= min_spp && taken % 4 == 0) {
        const double n = (double)taken;
        double var_of_mean = (ps.lum_sq - ps.lum_sum * ps.lum_sum / n) / (n - 1.0) / n;
        if (!(var_of_mean > 0.0)) var_of_mean = 0.0;
        double mean = ps.lum_sum / n;
        if (!(mean > 1e-4)) mean = 1e-4;
        if (sqrt(var_of_mean) / mean < threshold) stopped = true;
      }
    }
    film[p] = acc;
    stats[p] = ps;
    state[p] = taken | (stopped ? 0x80000000u : 0u);
  }
}
// The pixels still sampling, as a list of owned-pixel indices (order irrelevant: every pixel is independent).
__global__ __launch_bounds__(kBlock) void k_compact_active(const uint32_t *state, uint32_t n_pix, uint32_t *active,
                                                           uint32_t *count) {
  for (uint32_t base = blockIdx.x * kBlock; base < n_pix; base += gridDim.x * kBlock) {
    const uint32_t p = base + threadIdx.x;
    const bool on = p < n_pix && (state[p] >> 31) == 0;
    const unsigned long long m = __ballot(on);
    if (m == 0) continue;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t at = 0;
    if (lane == leader) at = atomicAdd(count, (uint32_t)__popcll(m));
    at = __shfl(at, leader, 64) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (on) active[at] = p;
  }
}

// pixel = sum / weight_sum (tracer.rs:630-634); rgb interleaved per owned pixel.
__global__ __launch_bounds__(kBlock) void k_film_out(const float4 *film, uint32_t n_pix, float *rgb) {
  for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < n_pix; p += gridDim.x * kBlock) {
    const float4 v = film[p];
    // weight_sum > 0 always holds for box/triangle (w = taken); the fallback arm divides by `taken` = w too.
    rgb[3 * (size_t)p] = v.x / v.w; rgb[3 * (size_t)p + 1] = v.y / v.w; rgb[3 * (size_t)p + 2] = v.z / v.w;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// The instance table: every instance of the multi-form kernels this build holds, named once — the lists of
// launch_plan.h expanded to rows {key, kernel}, one typed pointer per kernel signature. A launch plan names keys
// (plan_launches); a key without a row is an error, never another instance. The host (render.cpp) sees none of it:
// it gets the pointers from resolve_kernels, the single-form kernels from kStageKernels (render_kernels.h).
// ---------------------------------------------------------------------------------------------
template <class Fn>
struct InstanceRow { InstanceKey key; Fn fn; };
#define CRT_ROW(family, kernel, ...) {CRT_INSTANCE_KEY(family, kernel, __VA_ARGS__), kernel<__VA_ARGS__>},
static const InstanceRow<ExtendFn> kExtendRows[] = {CRT_INSTANCES_EXTEND(CRT_ROW)};
static const InstanceRow<ExtendDeferredFn> kExtendDeferredRows[] = {CRT_INSTANCES_EXTEND_DEFERRED(CRT_ROW)};
static const InstanceRow<PathFn> kPathRows[] = {CRT_INSTANCES_PATH(CRT_ROW)};
static const InstanceRow<ShadeFn> kShadeRows[] = {CRT_INSTANCES_SHADE(CRT_ROW)};
static const InstanceRow<ShadePipeFn> kShadePipeRows[] = {CRT_INSTANCES_SHADE_PIPE(CRT_ROW) CRT_INSTANCES_SHADE_PIPE_SLIM(CRT_ROW)};
static const InstanceRow<ShadowFn> kShadowRows[] = {CRT_INSTANCES_SHADOW(CRT_ROW)};
static const InstanceRow<ShadeVolFn> kShadeVolRows[] = {CRT_INSTANCES_SHADE_VOL(CRT_ROW)};
static const InstanceRow<ExtendFacesFn> kExtendFacesRows[] = {CRT_INSTANCES_EXTEND_FACES(CRT_ROW)};
static const InstanceRow<ShadeFacesFn> kShadeFacesRows[] = {CRT_INSTANCES_SHADE_FACES(CRT_ROW)};
static const InstanceRow<ShadeGuidedFn> kShadeGuidedRows[] = {CRT_INSTANCES_SHADE_GUIDED(CRT_ROW)};
static const InstanceRow<CameraFn> kCameraRows[] = {CRT_INSTANCES_CAMERA(CRT_ROW)};
static const InstanceRow<CameraVertexFn> kCameraVertexRows[] = {CRT_INSTANCES_CAMERA_VERTEX(CRT_ROW)};
#undef CRT_ROW
// The kernel a key names (nullptr for the empty key: nothing to launch); false when the build holds no such instance.
template <class Fn, size_t N>
static bool find_instance(const InstanceRow<Fn> (&rows)[N], const InstanceKey &key, Fn &fn) {
  fn = nullptr;
  if (key.none()) return true;
  for (const InstanceRow<Fn> &r : rows)
    if (r.key == key) { fn = r.fn; return true; }
  set_error_text("render refused: no such instance in this build (family %d: %d, %d, %d, %d, %d)", (int)key.family, (int)key.arg[0],
                 (int)key.arg[1], (int)key.arg[2], (int)key.arg[3], (int)key.arg[4]);
  return false;
}
int resolve_kernels(const LaunchPlan &plan, BatchKernels &k) {
  k = BatchKernels{};
  if (plan.volumes && !find_instance(kShadeVolRows, plan.shade, k.shade_vol)) return CRT_ERR_UNSUPPORTED;
  if (plan.volumes && (plan.volume_key.none() || plan.fused)) return CRT_ERR_UNSUPPORTED;
  if (plan.faces) {  // textured renders: the two FACES instances in the place of extend and shade, per stage, nothing else new
    if (plan.volumes || plan.fused || plan.camera_trace || plan.shade_piped() || !plan.path.none()) return CRT_ERR_UNSUPPORTED;
    if (!find_instance(kExtendFacesRows, plan.extend, k.extend_faces) || !find_instance(kShadeFacesRows, plan.shade, k.shade_faces) ||
        !find_instance(kShadowRows, plan.shadow_key, k.shadow) || !k.extend_faces || !k.shade_faces)
      return CRT_ERR_UNSUPPORTED;
    return CRT_OK;
  }
  if (plan.guided) {  // guided renders: the GUIDED instance in the place of shade, per stage, nothing else new
    if (plan.volumes || plan.fused || plan.camera_trace || plan.cam_compact || plan.shade_piped() || !plan.path.none()) return CRT_ERR_UNSUPPORTED;
    if (!find_instance(kExtendRows, plan.extend, k.extend) || !find_instance(kShadeGuidedRows, plan.shade, k.shade_guided) ||
        !find_instance(kShadowRows, plan.shadow_key, k.shadow) || !k.extend || !k.shade_guided)
      return CRT_ERR_UNSUPPORTED;
    return CRT_OK;
  }
  const InstanceKey camera = plan.camera_key();
  if (!find_instance(kPathRows, plan.path, k.path) || !find_instance(kExtendRows, plan.extend, k.extend) ||
      (!plan.volumes && !find_instance(kShadeRows, plan.shade, k.shade)) || !find_instance(kShadePipeRows, plan.shade_early, k.shade_pipe) ||
      !find_instance(kShadePipeRows, plan.shade_slim_key(), k.shade_slim) ||
      !find_instance(kShadowRows, plan.shadow_key, k.shadow) ||
      !find_instance(kExtendDeferredRows, plan.extend_deferred_key(), k.extend_deferred) ||
      !(camera.family == KF_CAMERA_VERTEX ? find_instance(kCameraVertexRows, camera, k.camera_vertex) : find_instance(kCameraRows, camera, k.camera)))
    return CRT_ERR_UNSUPPORTED;
  if (plan.camera_trace && (!k.extend_deferred || plan.cam_compact == 0 || plan.fused)) return CRT_ERR_UNSUPPORTED;
  return CRT_OK;
}

const KernelBuild kKernelBuild = {sizeof(DevMaterial), sizeof(DevMedium), sizeof(PixelRec), mat_lds_max(kArenaDwords), kPipeMatMax,
                                  kRootCullBuild, kShadePipeBuild, kRegenFirst, CRT_CAM_COMPACT_BUILD != 0, CRT_MAT_INDEX_BUILD != 0};
const StageKernels kStageKernels = {k_generate, k_volume, k_shadow_volume, k_resolve, k_resolve_adaptive, k_compact_active, k_film_out,
                                    k_fill_pixel_table, k_derive_materials, k_build_media, k_number_media};

}  // namespace crt
