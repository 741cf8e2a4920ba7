// The device source of the camera rays' one-ray-per-lane traversal (kernels/traverse_camera.hip.h: camera_trace,
// camera_hit_record) compiled as host C++ for tests/test_camera_trace_host.py, behind the stand-in <hip/hip_runtime.h> of
// profiles/host_shade. The image is the one the library would upload (crt_scene_image_array); no window is staged
// (n_lds = 0: every node and packet is read from the arrays — the two arms hold the same expressions).
#include <hip/hip_runtime.h>

static inline uint32_t __shfl_down(uint32_t v, unsigned, int) { return v; }
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) {
  const unsigned long long old = *p;
  *p += v;
  return old;
}

#include "traverse_camera.hip.h"

extern "C" {
// view: root, has_packets, n_nodes, n_packets, direct_leaves, pool_stack, cold, 0 (crt_scene_image_array).
// Per ray of six floats: status (CAM_MISS 0 / CAM_HIT 1 / CAM_DEFER 2), the hit record's four floats and geometry word
// as the kernel stores them, the node and packet steps taken.
void camera_host_trace_n(const void *nodes, const void *leaves, const void *packets, const void *indices, const void *prims,
                         const void *instances, const void *normals, const uint32_t view[8], const float *rays6, size_t n,
                         uint32_t pstack, uint32_t rmask, float t_min, float t_max, int32_t *status, float *hit4,
                         uint32_t *geom_word, uint32_t *steps2) {
  using namespace crt;
  using namespace crt::dev;
  DevScene S{};
  S.nodes = static_cast<const WideNode *>(nodes); S.leaves = static_cast<const Leaf *>(leaves);
  S.packets = static_cast<const Tri4 *>(packets); S.indices = static_cast<const uint32_t *>(indices);
  S.prims = static_cast<const DevPrim *>(prims); S.instances = static_cast<const DevInstance *>(instances);
  S.normals = static_cast<const float *>(normals);
  S.root = view[0]; S.has_packets = view[1]; S.n_nodes = view[2]; S.n_packets = view[3]; S.direct_leaves = view[4];
  S.pool_stack = view[5]; S.cold = view[6];
  uint32_t stack[kCamStack];
  if (pstack > (uint32_t)kCamStack) pstack = (uint32_t)kCamStack;
  for (size_t i = 0; i < n; i++) {
    const float *r = rays6 + 6 * i;
    float t = 0.0f;
    uint32_t prim = kInvalid;
    CamSteps st{0, 0};
    const int res = camera_trace<true>(S, nullptr, 0u, 0u, stack, 1, pstack, t_min, t_max, rmask, r[0], r[1], r[2], r[3], r[4], r[5],
                                       t, prim, &st);
    status[i] = res;
    steps2[2 * i] = st.nodes; steps2[2 * i + 1] = st.packets;
    float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t gw = kInvalid;
    if (res == CAM_HIT) camera_hit_record(S, prim, t, r[3], r[4], r[5], h, gw);
    hit4[4 * i] = h.x; hit4[4 * i + 1] = h.y; hit4[4 * i + 2] = h.z; hit4[4 * i + 3] = h.w;
    geom_word[i] = gw;
  }
}
int camera_host_stack_entries() { return crt::dev::kCamStack; }
}
