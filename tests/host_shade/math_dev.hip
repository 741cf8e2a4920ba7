// Device drivers for kernels/dmath.hip.h and kernels/qmc.hip.h (tests only): one small kernel per function over arrays,
// behind extern "C" launchers that take device pointers and a count, so tests/test_gpu_math.py can compare what gfx950
// computes with the oracle (oracle/ora_mathdrv.c) and, for the bare arithmetic, with numpy. The host build of the same
// list is math_host.cpp. Built by tests/math_drivers.py with the flags `make -C crust-render_amd/csrc print-hipflags`
// reports, i.e. the product's own; nothing here is linked into libcrt_amd.so.
// Every launcher returns the hipError_t of launch + synchronize (0 = ok).
#include <hip/hip_runtime.h>
#include "math_ops.h"

using namespace crt_math_test;

namespace {
constexpr int kBlock = 256;
inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
inline int finish() {
  const hipError_t e = hipGetLastError();
  const hipError_t s = hipDeviceSynchronize();
  return (int)(e != hipSuccess ? e : s);
}
__device__ __forceinline__ size_t elem() { return (size_t)blockIdx.x * kBlock + threadIdx.x; }
}  // namespace

#define D1(name, TI, TO, expr)                                                                     \
  __global__ void k_m_##name(const TI *__restrict__ a, size_t n, TO *__restrict__ o) {             \
    const size_t i = elem();                                                                       \
    if (i < n) o[i] = (expr);                                                                      \
  }                                                                                                \
  extern "C" int dev_m_##name##_n(const TI *a, size_t n, TO *o) {                                  \
    if (n == 0) return 0;                                                                          \
    hipLaunchKernelGGL(k_m_##name, grid_for(n), dim3(kBlock), 0, nullptr, a, n, o);                \
    return finish();                                                                               \
  }
#define D2(name, TA, TB, TO, expr)                                                                 \
  __global__ void k_m_##name(const TA *__restrict__ a, const TB *__restrict__ b, size_t n, TO *__restrict__ o) { \
    const size_t i = elem();                                                                       \
    if (i < n) o[i] = (expr);                                                                      \
  }                                                                                                \
  extern "C" int dev_m_##name##_n(const TA *a, const TB *b, size_t n, TO *o) {                     \
    if (n == 0) return 0;                                                                          \
    hipLaunchKernelGGL(k_m_##name, grid_for(n), dim3(kBlock), 0, nullptr, a, b, n, o);             \
    return finish();                                                                               \
  }
#define D3(name, T, expr)                                                                          \
  __global__ void k_m_##name(const T *__restrict__ a, const T *__restrict__ b, const T *__restrict__ c, size_t n, \
                             T *__restrict__ o) {                                                  \
    const size_t i = elem();                                                                       \
    if (i < n) o[i] = (expr);                                                                      \
  }                                                                                                \
  extern "C" int dev_m_##name##_n(const T *a, const T *b, const T *c, size_t n, T *o) {            \
    if (n == 0) return 0;                                                                          \
    hipLaunchKernelGGL(k_m_##name, grid_for(n), dim3(kBlock), 0, nullptr, a, b, c, n, o);          \
    return finish();                                                                               \
  }
CRT_MATH_OPS(D1, D2, D3)

__global__ void k_m_sincos(const float *__restrict__ a, size_t n, float *__restrict__ s, float *__restrict__ c) {
  const size_t i = elem();
  if (i < n) sincos_det(a[i], s[i], c[i]);
}
__global__ void k_m_dot(const float *__restrict__ a, const float *__restrict__ b, size_t n, float *__restrict__ o) {
  const size_t i = elem();
  if (i < n) o[i] = dot(v3(a[3 * i], a[3 * i + 1], a[3 * i + 2]), v3(b[3 * i], b[3 * i + 1], b[3 * i + 2]));
}
__global__ void k_m_normalize(const float *__restrict__ a, size_t n, float *__restrict__ o) {
  const size_t i = elem();
  if (i < n) {
    const V3 r = normalize(v3(a[3 * i], a[3 * i + 1], a[3 * i + 2]));
    o[3 * i] = r.x; o[3 * i + 1] = r.y; o[3 * i + 2] = r.z;
  }
}
__global__ void k_m_sampler_new(const int32_t *__restrict__ a, size_t n, uint32_t *__restrict__ pattern) {
  const size_t i = elem();
  if (i < n) pattern[i] = sampler_new(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]).pattern;
}
// The byte-sliced Sobol table lives in LDS, filled by the block, as in k_shade / k_path.
__global__ void k_m_draw_sample4(const uint32_t *__restrict__ pattern, const uint32_t *__restrict__ index, size_t n,
                                 float *__restrict__ o) {
  __shared__ uint32_t tab[kSobolLdsWords];
  sobol_tables_init(tab);
  const size_t i = elem();
  if (i < n) {
    float r[4];
    draw_sample4(Sampler{pattern[i], index[i]}, r, tab);
    o[4 * i] = r[0]; o[4 * i + 1] = r[1]; o[4 * i + 2] = r[2]; o[4 * i + 3] = r[3];
  }
}
__global__ void k_m_sobol_dirs(uint32_t *__restrict__ o) {
  if (threadIdx.x < 128) o[threadIdx.x] = kSobolDirs[threadIdx.x >> 5][threadIdx.x & 31];
}
__global__ void k_m_sobol_table(uint32_t *__restrict__ o) {
  __shared__ uint32_t tab[kSobolLdsWords];
  sobol_tables_init(tab);
  for (int e = threadIdx.x; e < kSobolLdsWords; e += kBlock) o[e] = tab[e];
}

extern "C" {
int dev_m_sincos_n(const float *a, size_t n, float *s, float *c) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_m_sincos, grid_for(n), dim3(kBlock), 0, nullptr, a, n, s, c);
  return finish();
}
int dev_m_dot_n(const float *a, const float *b, size_t n, float *o) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_m_dot, grid_for(n), dim3(kBlock), 0, nullptr, a, b, n, o);
  return finish();
}
int dev_m_normalize_n(const float *a, size_t n, float *o) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_m_normalize, grid_for(n), dim3(kBlock), 0, nullptr, a, n, o);
  return finish();
}
int dev_m_sampler_new_n(const int32_t *a, size_t n, uint32_t *pattern) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_m_sampler_new, grid_for(n), dim3(kBlock), 0, nullptr, a, n, pattern);
  return finish();
}
int dev_m_draw_sample4_n(const uint32_t *pattern, const uint32_t *index, size_t n, float *o) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_m_draw_sample4, grid_for(n), dim3(kBlock), 0, nullptr, pattern, index, n, o);
  return finish();
}
int dev_m_sobol_dirs(uint32_t *o /* 4 * 32 */) {
  hipLaunchKernelGGL(k_m_sobol_dirs, dim3(1), dim3(kBlock), 0, nullptr, o);
  return finish();
}
int dev_m_sobol_table(uint32_t *o /* kSobolLdsWords */) {
  hipLaunchKernelGGL(k_m_sobol_table, dim3(1), dim3(kBlock), 0, nullptr, o);
  return finish();
}
}  // extern "C"
