// What the unsharp-mask kernels (usm.hip: k_usm_pass) and their host twin (srk_usm_u8_host) share: the reflect-101
// index, the K-tap sum in index order and the two epilogues.  One body, compiled for both sides, products and sums
// uncontracted so that both make the same roundings.  DESIGN.md 32.
#ifndef SRK_USM_COMMON_H_
#define SRK_USM_COMMON_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace srk {

constexpr int kUsmMaxK = 51;

// Reflect-101 of a coordinate first clamped to [-r, n - 1 + r] (n > r): what lies further out belongs to outputs past the
// plane's edge, which are never stored, and must only stay inside the plane.
__host__ __device__ __forceinline__ int usm_reflect(int c, int n, int r) {
  c = c < -r ? -r : (c > n - 1 + r ? n - 1 + r : c);
  return c < 0 ? -c : (c >= n ? 2 * (n - 1) - c : c);
}

// sum_t g[t] * v[t * stride], t = 0 .. K - 1 in that order from 0.0.
template <typename T>
__host__ __device__ __forceinline__ double usm_taps(const double* g, const T* v, int stride, int K) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int t = 0; t < K; ++t) acc = acc + g[t] * (double)v[t * stride];
  return acc;
}

// First half: the residual R = P - Bl and the mask |R| > threshold.
__host__ __device__ __forceinline__ void usm_residual(uint8_t p, double bl, double threshold, double* r, uint8_t* m) {
  *r = (double)p - bl;
  *m = fabs(*r) > threshold ? 1 : 0;
}

// Second half: the soft mask S blends the sharpened level into the pixel.
__host__ __device__ __forceinline__ uint8_t usm_finish(uint8_t p, double r, double s, double weight) {
#pragma clang fp contract(off)
  const double P = (double)p;
  const double sharp = fmin(fmax(P + weight * r, 0.0), 255.0);
  const double a = s * sharp, b = (1.0 - s) * P;
  return (uint8_t)(int)floor(fmin(fmax(a + b, 0.0), 255.0) + 0.5);
}

}  // namespace srk
#endif  // SRK_USM_COMMON_H_
