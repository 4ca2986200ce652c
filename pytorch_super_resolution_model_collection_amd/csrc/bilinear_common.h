// Bilinear x2 upsampling (F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)) as the kernels
// (bilinear.hip) and their host twin both index it: the source pair and the weights of one output coordinate, and the
// weight an output coordinate gives one input coordinate (the adjoint).  The weights 0.25 / 0.75 / 1 are exact in binary.
#ifndef SRK_BILINEAR_COMMON_H_
#define SRK_BILINEAR_COMMON_H_
#include <hip/hip_runtime.h>

namespace srk {

// Output coordinate o of an axis of n inputs (0 <= o < 2 n) reads i0 and i1 with weights w0 and w1:
//   o = 2 k      (k - 1, k)               (0.25, 0.75), and index 0 alone for k = 0
//   o = 2 k + 1  (k, min(k + 1, n - 1))   (0.75, 0.25)
template <typename T>
__host__ __device__ __forceinline__ void bilinear2x_src(int o, int n, int* i0, int* i1, T* w0, T* w1) {
  const int k = o >> 1;
  if (o & 1) {
    *i0 = k, *i1 = k + 1 < n ? k + 1 : n - 1;
    *w0 = (T)0.75, *w1 = (T)0.25;
  } else if (k == 0) {
    *i0 = 0, *i1 = 0;
    *w0 = (T)1, *w1 = (T)0;
  } else {
    *i0 = k - 1, *i1 = k;
    *w0 = (T)0.25, *w1 = (T)0.75;
  }
}

// The weight with which output coordinate o reads input coordinate i (0 where it does not, or where o is outside
// [0, 2 n)).  The outputs that read i lie in 2 i - 1 .. 2 i + 2.
template <typename T>
__host__ __device__ __forceinline__ T bilinear2x_adj(int o, int i, int n) {
  if (o < 0 || o >= 2 * n) return (T)0;
  int i0, i1;
  T w0, w1;
  bilinear2x_src<T>(o, n, &i0, &i1, &w0, &w1);
  return (i0 == i ? w0 : (T)0) + (i1 == i ? w1 : (T)0);
}

// One output value from its four sources, in the order torch's kernel adds them.
template <typename T>
__host__ __device__ __forceinline__ T bilinear2x_mix(T x00, T x01, T x10, T x11, T wy0, T wy1, T wx0, T wx1) {
  return wy0 * (wx0 * x00 + wx1 * x01) + wy1 * (wx0 * x10 + wx1 * x11);
}

}  // namespace srk
#endif  // SRK_BILINEAR_COMMON_H_
