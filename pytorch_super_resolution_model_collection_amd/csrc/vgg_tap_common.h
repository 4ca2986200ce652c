// What the VGG tap kernels (vgg_tap.hip: k_vgg_tap_fwd / k_vgg_tap_bwd) and their host twins (srk_vgg_tap_forward_host /
// srk_vgg_tap_backward_host) share: the body of one 2 x 2 window of one channel, and of one element.  One body, compiled
// for both sides; T is the type the gradient is formed in before its fp32 store (float on the device, double on the
// host).  The loss term of an element is |a - b| with the difference taken in double on both sides.  DESIGN.md 33.
#ifndef SRK_VGG_TAP_COMMON_H_
#define SRK_VGG_TAP_COMMON_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace srk {

constexpr int kVggTapPartials = 1024;   // fp64 partial slots of one tap's row: the grid cap of the tap kernels

// |a - b| of one element, the difference in double (exact for fp32 operands up to its one rounding).
__host__ __device__ __forceinline__ double vgg_tap_term(float a, float b) { return fabs((double)a - (double)b); }

// sign(a - b) with sign(0) = 0
template <typename T>
__host__ __device__ __forceinline__ T vgg_tap_sign(float a, float b) {
  return a > b ? (T)1 : (a < b ? (T)-1 : (T)0);
}

// The winner of a window under the rule of k_maxpool2_bwd: row, column order, only a strictly greater value
// replaces the running one.  v = {(0,0), (0,1), (1,0), (1,1)}; *m = its value.
__host__ __device__ __forceinline__ int vgg_tap_winner(const float v[4], float* m) {
  float best = v[0];
  int k = 0;
  if (v[1] > best) best = v[1], k = 1;
  if (v[2] > best) best = v[2], k = 2;
  if (v[3] > best) best = v[3], k = 3;
  *m = best;
  return k;
}

// pool(relu(v)) of one whole window: the maximum of the four, or 0 where that is not positive.
__host__ __device__ __forceinline__ float vgg_tap_pool_relu(const float v[4]) {
  float m;
  (void)vgg_tap_winner(v, &m);
  return m > 0.f ? m : 0.f;
}

// Forward of one window of one channel.  a, b: the four values of either map (a clamped copy where the window hangs over
// the plane's edge); has_x1 / has_y1: the window's second column / row lies inside the plane.  Returns the window's sum of
// |a - b| over the elements inside the plane; *pa, *pb: the pooled values (meaningful for a whole window only).
__host__ __device__ __forceinline__ double vgg_tap_window_fwd(const float a[4], const float b[4], bool has_x1, bool has_y1,
                                                              float* pa, float* pb) {
  double s = vgg_tap_term(a[0], b[0]);
  const double t1 = vgg_tap_term(a[1], b[1]), t2 = vgg_tap_term(a[2], b[2]), t3 = vgg_tap_term(a[3], b[3]);
  s += has_x1 ? t1 : 0.0;
  s += has_y1 ? t2 : 0.0;
  s += (has_x1 && has_y1) ? t3 : 0.0;
  *pa = vgg_tap_pool_relu(a);
  *pb = vgg_tap_pool_relu(b);
  return s;
}

// Backward of one window of one channel: da[i] = c * sign(a[i] - b[i]) + (i is the winner of a routing window ? g : 0).
// A window routes where it is whole and its maximum is positive (the ReLU in front of the pool).
template <typename T>
__host__ __device__ __forceinline__ void vgg_tap_window_bwd(const float a[4], const float b[4], float g, T c, bool whole,
                                                            float da[4]) {
  float m;
  const int k = vgg_tap_winner(a, &m);
  const T gi = (whole && m > 0.f) ? (T)g : (T)0;
#pragma unroll
  for (int i = 0; i < 4; ++i) da[i] = (float)(c * vgg_tap_sign<T>(a[i], b[i]) + (k == i ? gi : (T)0));
}

// One element behind a plain ReLU (relu = true, g = the gradient of relu(a)) or at the end of the head (relu = false).
template <typename T>
__host__ __device__ __forceinline__ float vgg_tap_elem_bwd(float a, float b, float g, T c, bool relu) {
  return (float)(c * vgg_tap_sign<T>(a, b) + ((relu && a > 0.f) ? (T)g : (T)0));
}

__host__ __device__ __forceinline__ float vgg_tap_relu(float v) { return v > 0.f ? v : 0.f; }

}  // namespace srk
#endif  // SRK_VGG_TAP_COMMON_H_
