// The relativistic average GAN loss of ESRGAN and its full gradient -- the two batch means included -- in one launch.
// Definition: include/srk.h and DESIGN.md 30; the per-sample term: ragan_common.h, shared with the host twin below.
//
//   k_ragan   one block of 256 threads: the two means, then the loss and the sums of dL/da and dL/db, then the two gradient
//             rows.  A thread adds its samples i = t, t + 256, ... in that order and the 256 partials meet in a tree over
//             LDS: the order is a function of B alone, so two calls give the same bits.  Everything is double up to the
//             fp32 stores.  B is a batch size: one block is all the parallelism there is to have.  No atomics.
#include "ragan_common.h"
#include "srk_common.h"

namespace srk {

constexpr int kRaganThreads = 256;

// the sum of v over the block, the same value in every thread; sh holds kRaganThreads doubles
__device__ __forceinline__ double ragan_block_sum(double v, double* sh) {
  __syncthreads();                  // the previous sum has been read
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = kRaganThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(kRaganThreads) void k_ragan(const float* __restrict__ real, const float* __restrict__ fake, int B,
                                                         double sgn, double grad_scale, float* __restrict__ loss,
                                                         float* __restrict__ d_real, float* __restrict__ d_fake) {
  __shared__ double sh[kRaganThreads];
  const int t = threadIdx.x;
  double sr = 0.0, sf = 0.0;
  for (int i = t; i < B; i += kRaganThreads) sr += (double)real[i], sf += (double)fake[i];
  const double mr = ragan_block_sum(sr, sh) / B;
  const double mf = ragan_block_sum(sf, sh) / B;
  double sl = 0.0, sa = 0.0, sb = 0.0;
  for (int i = t; i < B; i += kRaganThreads) {
    double da, db;
    sl += ragan_term(sgn, (double)real[i] - mf, (double)fake[i] - mr, &da, &db);
    sa += da, sb += db;
  }
  const double w = 0.5 / B;         // the 1 / 2B of the mean over both rows
  const double L = ragan_block_sum(sl, sh) * w;
  const double mean_a = ragan_block_sum(sa, sh) * w / B;
  const double mean_b = ragan_block_sum(sb, sh) * w / B;
  if (t == 0) *loss = (float)L;
  if (!d_real && !d_fake) return;
  for (int i = t; i < B; i += kRaganThreads) {
    double da, db;
    ragan_term(sgn, (double)real[i] - mf, (double)fake[i] - mr, &da, &db);
    if (d_real) d_real[i] = (float)(grad_scale * (da * w - mean_b));
    if (d_fake) d_fake[i] = (float)(grad_scale * (db * w - mean_a));
  }
}

}  // namespace srk

using namespace srk;

extern "C" int srk_ragan_loss_forward_backward(const float* real, const float* fake, int B, int for_generator,
                                               float grad_scale, float* loss, float* d_real, float* d_fake, void* workspace,
                                               void* stream) {
  const char* who = "ragan_loss_forward_backward";
  (void)workspace;
  SRK_REQUIRE(real && fake && loss, "%s: null pointer", who);
  SRK_REQUIRE(B >= 1, "%s: B = %d logits", who, B);
  hipLaunchKernelGGL(k_ragan, dim3(1), dim3(kRaganThreads), 0, (hipStream_t)stream, real, fake, B, for_generator ? 1.0 : -1.0,
                     (double)grad_scale, loss, d_real, d_fake);
  return check_launch(who);
}

extern "C" int srk_ragan_loss_host(const float* real, const float* fake, int B, int for_generator, double grad_scale,
                                   double* loss, double* d_real, double* d_fake) {
  const char* who = "ragan_loss_host";
  SRK_REQUIRE(real && fake && loss, "%s: null pointer", who);
  SRK_REQUIRE(B >= 1, "%s: B = %d logits", who, B);
  const double sgn = for_generator ? 1.0 : -1.0, w = 0.5 / B;
  double sr = 0.0, sf = 0.0;
  for (int i = 0; i < B; ++i) sr += (double)real[i], sf += (double)fake[i];
  const double mr = sr / B, mf = sf / B;
  double sl = 0.0, sa = 0.0, sb = 0.0;
  for (int i = 0; i < B; ++i) {
    double da, db;
    sl += ragan_term(sgn, (double)real[i] - mf, (double)fake[i] - mr, &da, &db);
    sa += da, sb += db;
  }
  *loss = sl * w;
  const double mean_a = sa * w / B, mean_b = sb * w / B;
  for (int i = 0; i < B; ++i) {
    double da, db;
    ragan_term(sgn, (double)real[i] - mf, (double)fake[i] - mr, &da, &db);
    if (d_real) d_real[i] = grad_scale * (da * w - mean_b);
    if (d_fake) d_fake[i] = grad_scale * (db * w - mean_a);
  }
  return SRK_OK;
}
