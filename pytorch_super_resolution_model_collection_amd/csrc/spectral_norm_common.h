// Spectral normalisation as the kernels (spectral_norm.hip) and their host twin (srk_spectral_norm_host) both compute it:
// the per-element formulas, in double.  Definition: include/srk.h and DESIGN.md 31.
#ifndef SRK_SPECTRAL_NORM_COMMON_H_
#define SRK_SPECTRAL_NORM_COMMON_H_
#include <hip/hip_runtime.h>
#include <math.h>

namespace srk {

// x / max(||x||, eps): one element of torch.nn.functional.normalize(x, dim=0, eps)
__host__ __device__ __forceinline__ double sn_normalized(double x, double norm, double eps) {
  return x / (norm > eps ? norm : eps);
}

// ||x|| from the sum of squares
__host__ __device__ __forceinline__ double sn_norm(double sumsq) { return sqrt(sumsq); }

// one element of w_sn = W / sigma
__host__ __device__ __forceinline__ double sn_weight(double w, double sigma) { return w / sigma; }

// one element of dW = (G - <G, w_sn> u v^T) / sigma
__host__ __device__ __forceinline__ double sn_grad(double g, double dot, double u, double v, double sigma) {
  return (g - dot * u * v) / sigma;
}

}  // namespace srk
#endif  // SRK_SPECTRAL_NORM_COMMON_H_
