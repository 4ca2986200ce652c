// The vanilla GAN loss on logits of any shape, mean softplus(-x) for a real target and mean softplus(x) for a fake one, with
// its gradient.  Definition: include/srk.h and DESIGN.md 31; softplus and the sigmoid: ragan_common.h, shared with k_ragan
// and with the host twin below.
//
//   k_gan_logit          one pass: a block adds softplus over its elements (grid-stride, a thread's elements in index
//                        order, then the block sum) into one double, and writes grad_scale * d loss / d x of each.
//   k_gan_logit_finish   one block: the partials in a fixed order, the mean, the fp32 store.
// The grid is a function of N alone, so two calls give the same bits.  Everything is double up to the fp32 stores; no atomics.
#include "ragan_common.h"
#include "srk_common.h"

namespace srk {

constexpr int kGlMaxBlocks = 1024;

static inline int gl_blocks(size_t n) { return (int)grid_for(n, 1024, kGlMaxBlocks); }

__global__ __launch_bounds__(256) void k_gan_logit(const float* __restrict__ x, size_t n, double sgn, double scale_over_n,
                                                   float* __restrict__ dx, double* __restrict__ part) {
  __shared__ double sm[4];
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double z = sgn * (double)x[i];           // real: sgn = -1, loss term softplus(-x); fake: sgn = +1
    acc += ragan_softplus(z);
    if (dx) dx[i] = (float)(scale_over_n * sgn * ragan_sigmoid(z));
  }
  store_block_sum_256_d(acc, sm, part + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_gan_logit_finish(const double* __restrict__ part, int nparts, double inv_n,
                                                          float* __restrict__ loss) {
  __shared__ double sm[4];
  const double tot = sum_partials_256_d(part, nparts, sm);
  if (threadIdx.x == 0) *loss = (float)(tot * inv_n);
}

}  // namespace srk

using namespace srk;

extern "C" size_t srk_gan_logit_loss_workspace_bytes(void) { return (size_t)kGlMaxBlocks * sizeof(double); }

extern "C" int srk_gan_logit_loss_forward_backward(const float* logits, size_t n, int target_is_real, float grad_scale,
                                                   float* loss, float* d_logits, void* workspace, void* stream) {
  const char* who = "gan_logit_loss_forward_backward";
  SRK_REQUIRE(logits && loss && workspace, "%s: null pointer", who);
  SRK_REQUIRE(n >= 1, "%s: n = %zu logits", who, n);
  SRK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: workspace is not 8-byte aligned", who);
  const int nb = gl_blocks(n);
  double* part = reinterpret_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gan_logit, dim3(nb), dim3(256), 0, s, logits, n, target_is_real ? -1.0 : 1.0,
                     (double)grad_scale / (double)n, d_logits, part);
  hipLaunchKernelGGL(k_gan_logit_finish, dim3(1), dim3(256), 0, s, (const double*)part, nb, 1.0 / (double)n, loss);
  return check_launch(who);
}

extern "C" int srk_gan_logit_loss_host(const float* logits, size_t n, int target_is_real, double grad_scale, double* loss,
                                       double* d_logits) {
  const char* who = "gan_logit_loss_host";
  SRK_REQUIRE(logits && loss, "%s: null pointer", who);
  SRK_REQUIRE(n >= 1, "%s: n = %zu logits", who, n);
  const double sgn = target_is_real ? -1.0 : 1.0, scale_over_n = grad_scale / (double)n;
  double acc = 0.0;
  for (size_t i = 0; i < n; ++i) {
    const double z = sgn * (double)logits[i];
    acc += ragan_softplus(z);
    if (d_logits) d_logits[i] = scale_over_n * sgn * ragan_sigmoid(z);
  }
  *loss = acc / (double)n;
  return SRK_OK;
}
