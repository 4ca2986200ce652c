// The relativistic average GAN loss as the kernel (ragan.hip) and its host twin (srk_ragan_loss_host) both compute it:
// one term of the sum and its two partial derivatives, in double.  Definition: include/srk.h and DESIGN.md 30.
#ifndef SRK_RAGAN_COMMON_H_
#define SRK_RAGAN_COMMON_H_
#include <hip/hip_runtime.h>
#include <math.h>

namespace srk {

// log(1 + exp(x)) without an overflow: the exponential's argument is never positive
__host__ __device__ __forceinline__ double ragan_softplus(double x) { return (x > 0.0 ? x : 0.0) + log1p(exp(-fabs(x))); }

// d softplus(x) / dx = 1 / (1 + exp(-x)), through the same never-positive exponent
__host__ __device__ __forceinline__ double ragan_sigmoid(double x) {
  const double t = exp(-fabs(x));
  return x >= 0.0 ? 1.0 / (1.0 + t) : t / (1.0 + t);
}

// One sample: a = real - mean(fake), b = fake - mean(real); sgn = +1 for the generator's loss, -1 for the discriminator's.
// Returns sp(sgn a) + sp(-sgn b); *da and *db are its derivatives with respect to a and b (the 1 / 2B is the caller's).
__host__ __device__ __forceinline__ double ragan_term(double sgn, double a, double b, double* da, double* db) {
  *da = sgn * ragan_sigmoid(sgn * a);
  *db = -sgn * ragan_sigmoid(-sgn * b);
  return ragan_softplus(sgn * a) + ragan_softplus(-sgn * b);
}

}  // namespace srk
#endif  // SRK_RAGAN_COMMON_H_
