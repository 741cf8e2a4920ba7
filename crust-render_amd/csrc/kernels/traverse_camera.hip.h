// Camera rays, one per lane: the closest-hit traversal of a ray in the lane that made it (pathtrace.hip, k_camera).
//
// Why not the pool engine (traverse_pool.hip.h) for these rays: the 64 camera rays of a wave are 64 consecutive pixels of
// one tile — they take the same node steps and reach the same leaves, so the phase scheduler has nothing to repair, and
// its machinery (the scheduling rounds, a ray's state going through LDS at fetch and again at emit, the ray itself going
// through HBM between generate and extend) is more than half of the first extend launch's cycles. A plain while-while
// loop over the ray's registers pays none of that.
//
// What it computes is the pool engine's per-ray sequence, expression for expression: the node step's slab4 with t_min and
// the closest hit so far, the six pairwise "is nearer" relations with lane order on equal keys, leaf lanes above inner
// lanes; the lean Tri4 test with the Woop order, the mask logic, the range test against the packet-entry bound, 1 / det
// for the lanes that hit, the accept rule in lane order against the running bound, the f64 re-evaluation of exact-zero
// edge functions behind the four lanes. So the visit order is the pool's for every ray, and the hit is the pool's bit for
// bit.
//
// What it does NOT do it DEFERS: a leaf with scalar entries (spheres, curves, instances), a direct leaf word, a stack
// deeper than the per-lane LDS part. A deferred ray is abandoned where it stands; the caller hands it to the pool engine,
// which traces it from the root — its result is then that engine's by construction.
//
// One source for the kernel and for the host build of the tests (tests/host_shade/camera_host.cpp, behind the stand-in
// <hip/hip_runtime.h>): the float contract of traverse.hip.h holds here too (-ffp-contract=off).
#pragma once

#include "traverse.hip.h"

namespace crt {
namespace dev {

constexpr int kCamStack = 8;     // stack entries per lane in LDS; a ray that needs more defers
constexpr int kCamWindow = 160;  // the staged top of the tree and its packets, in node strides (stage_nodes)
enum : int { CAM_MISS = 0, CAM_HIT = 1, CAM_DEFER = 2 };

#if defined(__HIPCC__)
// Opaque to the optimiser: keeps the LDS arm and the global arm of a load apart (merged they become FLAT loads through a
// generic pointer, traverse_pool.hip.h).
#define CRT_CAM_ARRIVED3(a, b, c) asm volatile("" : "+v"(a), "+v"(b), "+v"(c))
#define CRT_CAM_ARRIVED5(a, b, c, d, e) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e))
#else
#define CRT_CAM_ARRIVED3(a, b, c)
#define CRT_CAM_ARRIVED5(a, b, c, d, e)
#endif

// What a run did, for the tests of the host build: the steps the pool engine would count for the same ray.
struct CamSteps { uint32_t nodes, packets; };

// One ray against the top-level tree of S. stk: this lane's stack, entry e at stk[e * stride], pstack (<= what the caller
// reserved) entries deep. lds_nodes / n_lds / n_lds_pk: the window stage_nodes filled (n_lds = n_lds_pk = 0: none).
// CAM_HIT: t and the primitive (index into S.prims) of the closest hit. COUNT: fill `steps`.
template <bool COUNT = false>
__device__ __forceinline__ int camera_trace(const DevScene &S, const uint32_t *lds_nodes, uint32_t n_lds, uint32_t n_lds_pk,
                                            uint32_t *stk, int stride, uint32_t pstack, float t_min, float t_max, uint32_t rmask,
                                            float ox, float oy, float oz, float dx, float dy, float dz, float &t_out,
                                            uint32_t &prim_out, CamSteps *steps = nullptr) {
  RayCtx r;
  r.ox = ox; r.oy = oy; r.oz = oz; r.dx = dx; r.dy = dy; r.dz = dz;
  r.kx = 0; r.ky = 1; r.kz = 2; r.sx = r.sy = r.sz = 0.0f;
  setup_ray(r, true);  // as the pool's store_ray
  const int kx = r.kx, ky = r.ky, kz = r.kz;
  float closest = t_max;
  uint32_t best = kInvalid;  // the closest hit's primitive so far
  uint32_t sp = 0;
  bool defer = false;
  // cur: a node index, a leaf word (kLeafTag), or kInvalid = the ray is finished (or deferred)
  uint32_t cur = S.root;
  auto pop = [&]() { cur = sp == 0 ? kInvalid : stk[(int)(--sp) * stride]; };
  for (;;) {
    while (!(cur & kLeafTag)) {
      // ================= node expansion (bvh.rs:455-505), as traverse_pool's =================
      if (COUNT) steps->nodes++;
      float4 mnx, mny, mnz, mxx, mxy, mxz;
      uint4 ch;
      if (cur < n_lds) {
        const float4 *nb = reinterpret_cast<const float4 *>(lds_nodes + (size_t)cur * kLdsNodeStride);
        mnx = nb[0]; mny = nb[1]; mnz = nb[2]; mxx = nb[3]; mxy = nb[4]; mxz = nb[5];
        ch = *reinterpret_cast<const uint4 *>(nb + 6);
        CRT_CAM_ARRIVED3(mnx.x, mxx.x, ch.x);
      } else {
        const WideNode *nd = &S.nodes[cur];
        const float4 *nb = reinterpret_cast<const float4 *>(nd);
        mnx = nb[0]; mny = nb[1]; mnz = nb[2]; mxx = nb[3]; mxy = nb[4]; mxz = nb[5];
        ch = *reinterpret_cast<const uint4 *>(nd->child);
      }
      const float lo_x[4] = {mnx.x, mnx.y, mnx.z, mnx.w}, lo_y[4] = {mny.x, mny.y, mny.z, mny.w},
                  lo_z[4] = {mnz.x, mnz.y, mnz.z, mnz.w};
      const float hi_x[4] = {mxx.x, mxx.y, mxx.z, mxx.w}, hi_y[4] = {mxy.x, mxy.y, mxy.z, mxy.w},
                  hi_z[4] = {mxz.x, mxz.y, mxz.z, mxz.w};
      const uint32_t child[4] = {ch.x, ch.y, ch.z, ch.w};
      float key[4];
      uint32_t ent[4];
#pragma unroll
      for (int l = 0; l < 4; l++) {  // RaySlab::slab4, bvh.rs:790-808
        const float t0x = (lo_x[l] - r.ox) * r.ix, t1x = (hi_x[l] - r.ox) * r.ix;
        const float t0y = (lo_y[l] - r.oy) * r.iy, t1y = (hi_y[l] - r.oy) * r.iy;
        const float t0z = (lo_z[l] - r.oz) * r.iz, t1z = (hi_z[l] - r.oz) * r.iz;
        const float tn = fmaxf(fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z)), t_min);
        const float tf = fminf(fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z)), closest);
        key[l] = tn;
        ent[l] = (tn <= tf) ? child[l] : kInvalid;
      }
      // the stack image after this node: inner lanes far to near, leaf lanes far to near on top (traverse_pool.hip.h)
      uint32_t on[4], lf4[4], pos[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { on[i] = ent[i] != kInvalid ? 1u : 0u; lf4[i] = (on[i] && (ent[i] & kLeafTag)) ? 1u : 0u; pos[i] = 0; }
#pragma unroll
      for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int j = i + 1; j < 4; j++) {
          const uint32_t a = key[i] <= key[j] ? 1u : 0u;
          const uint32_t t = lf4[i] ^ lf4[j];
          const uint32_t x = (t & lf4[i]) | (~t & a);
          pos[i] += on[j] & x;
          pos[j] += on[i] & (x ^ 1u);
        }
      }
      const uint32_t n_tot = on[0] + on[1] + on[2] + on[3];
      if (n_tot == 0) { pop(); continue; }
      if (sp + n_tot - 1 > pstack) { defer = true; cur = kInvalid; break; }  // deeper than the LDS part
      uint32_t top_e = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (on[i]) {
          if (pos[i] == n_tot - 1) top_e = ent[i];
          else stk[(int)(sp + pos[i]) * stride] = ent[i];
        }
      }
      sp += n_tot - 1;
      cur = top_e;
    }
    if (cur == kInvalid) break;
    // ============ the Tri4 packets of leaf `cur` (bvh.rs:514-562, triangle.rs:276-348) ============
    if (cur & kDirectLeafTag) { defer = true; break; }  // a direct leaf word: the scalar list itself
    Leaf lf;
    {
      uint4 lw = *reinterpret_cast<const uint4 *>(&S.leaves[cur & ~kLeafTag]);
      lf.pkt_first = lw.x; lf.pkt_count = lw.y; lf.idx_first = lw.z; lf.idx_count = lw.w;
    }
    if (lf.idx_count > 0) { defer = true; break; }  // scalar entries: spheres, curves, instances
    for (uint32_t k = 0; k < lf.pkt_count; k++) {
      if (COUNT) steps->packets++;
      const uint32_t pki = lf.pkt_first + k;
      const bool pk_lds = pki < n_lds_pk;
      const Tri4 *pk = &S.packets[pki];
      const Tri4 *pk_l = reinterpret_cast<const Tri4 *>(lds_nodes + (size_t)n_lds * kLdsNodeStride) + (pk_lds ? pki : 0u);
      uint4 prim4;
      uint32_t normal_ok, m;
      float4 A_x, A_y, A_z, B_x, B_y, B_z, C_x, C_y, C_z;
      uint32_t am_x, am_y;  // active, mask_and
      auto load_lean = [&](const Tri4 *q) {
        am_x = q->active; am_y = q->mask_and;
        prim4 = *reinterpret_cast<const uint4 *>(q->prim);
        normal_ok = q->normal_ok;
        const float4 *pl = reinterpret_cast<const float4 *>(q);
        A_x = pl[0 + kx]; A_y = pl[0 + ky]; A_z = pl[0 + kz];
        B_x = pl[3 + kx]; B_y = pl[3 + ky]; B_z = pl[3 + kz];
        C_x = pl[6 + kx]; C_y = pl[6 + ky]; C_z = pl[6 + kz];
      };
      if (pk_lds) { load_lean(pk_l); CRT_CAM_ARRIVED5(A_x.x, B_x.x, C_x.x, prim4.x, am_x); }
      else load_lean(pk);
      if (rmask & am_y) m = am_x;                                        // triangle.rs:257-271
      else if ((rmask & (pk_lds ? pk_l->mask_or : pk->mask_or)) == 0) m = 0;
      else {
        m = 0;
#pragma unroll
        for (int l = 0; l < 4; l++)
          if ((am_x & (1u << l)) && ((pk_lds ? pk_l->masks[l] : pk->masks[l]) & rmask)) m |= 1u << l;
      }
      if (m == 0) continue;
      const uint32_t prim_of[4] = {prim4.x, prim4.y, prim4.z, prim4.w};
      const float vax[4] = {A_x.x, A_x.y, A_x.z, A_x.w}, vay[4] = {A_y.x, A_y.y, A_y.z, A_y.w}, vaz[4] = {A_z.x, A_z.y, A_z.z, A_z.w};
      const float vbx[4] = {B_x.x, B_x.y, B_x.z, B_x.w}, vby[4] = {B_y.x, B_y.y, B_y.z, B_y.w}, vbz[4] = {B_z.x, B_z.y, B_z.z, B_z.w};
      const float vcx[4] = {C_x.x, C_x.y, C_x.z, C_x.w}, vcy[4] = {C_y.x, C_y.y, C_y.z, C_y.w}, vcz[4] = {C_z.x, C_z.y, C_z.z, C_z.w};
      uint32_t fallback = 0;
      const float entry_closest = closest;  // every lane range-tests against the packet-entry bound
      // One triangle after another: a lane's test reads the packet-entry bound, its accept the running one — what the
      // pool's test-all-then-accept-in-lane-order sees, lane by lane.
#pragma unroll
      for (int l = 0; l < 4; l++) {  // triangle.rs:284-347
        const float akz = vaz[l] - r.okz, bkz = vbz[l] - r.okz, ckz = vcz[l] - r.okz;
        const float ax = (vax[l] - r.okx) - r.sx * akz, ay = (vay[l] - r.oky) - r.sy * akz;
        const float bx = (vbx[l] - r.okx) - r.sx * bkz, by = (vby[l] - r.oky) - r.sy * bkz;
        const float cx = (vcx[l] - r.okx) - r.sx * ckz, cy = (vcy[l] - r.oky) - r.sy * ckz;
        const float e0 = bx * cy - by * cx;
        const float e1 = cx * ay - cy * ax;
        const float e2 = ax * by - ay * bx;
        const bool zero = (e0 == 0.0f) | (e1 == 0.0f) | (e2 == 0.0f);
        const bool neg = (e0 < 0.0f) | (e1 < 0.0f) | (e2 < 0.0f);
        const bool posv = (e0 > 0.0f) | (e1 > 0.0f) | (e2 > 0.0f);
        const float det = e0 + e1 + e2;
        const float t_scaled = e0 * (r.sz * akz) + e1 * (r.sz * bkz) + e2 * (r.sz * ckz);
        const float abs_det = absf(det);
        const float ts = det < 0.0f ? -t_scaled : t_scaled;
        const bool in_range = (ts >= t_min * abs_det) & (ts <= entry_closest * abs_det);
        const bool lane_on = (m >> l) & 1u;
        if (lane_on && zero) fallback |= 1u << l;
        if (lane_on && !zero && !(neg && posv) && det != 0.0f && in_range) {  // bvh.rs:533-550
          const float inv_det = 1.0f / det;  // triangle.rs:339-343, the IEEE division
          const float t = t_scaled * inv_det;
          if (!(t > closest) && ((normal_ok >> l) & 1u)) {  // strict: an exact tie goes to the later lane; prim.rs:81-83
            closest = t;
            best = prim_of[l];
          }
        }
      }
      if (fallback) {  // bvh.rs:551-561 — lanes sitting exactly on an edge, behind the four
#pragma unroll
        for (int l = 0; l < 4; l++) {
          if (!((fallback >> l) & 1u)) continue;
          const uint32_t pi = prim_of[l];
          const DevPrim *p = &S.prims[pi];
          if ((rmask & p->mask) == 0) continue;
          float t, u, v;
          if (!tri_scalar(r, p->d, t_min, closest, t, u, v)) continue;
          if (!((normal_ok >> l) & 1u)) continue;
          closest = t;
          best = pi;
        }
      }
    }
    pop();
  }
  if (defer) return CAM_DEFER;
  if (best == kInvalid) return CAM_MISS;
  t_out = closest;
  prim_out = best;
  return CAM_HIT;
}

// The hit record of a closest hit as extend_segment's emit writes it: t and the ray-facing normal, the geometry id with
// the front-face bit (scene.rs:356-359). Flat triangles only: the caller's image holds no shading normal (cold state 0).
__device__ __forceinline__ void camera_hit_record(const DevScene &S, uint32_t prim, float t, float dx, float dy, float dz,
                                                  float4 &h, uint32_t &geom_word) {
  float nx, ny, nz;
  tri_normal<false>(S, prim, 0.0f, 0.0f, nx, ny, nz);
  const bool front = dot3(dx, dy, dz, nx, ny, nz) < 0.0f;
  h = make_float4(t, front ? nx : -nx, front ? ny : -ny, front ? nz : -nz);
  geom_word = S.prims[prim].geom_id | (front ? 0x80000000u : 0u);
}

}  // namespace dev
}  // namespace crt
