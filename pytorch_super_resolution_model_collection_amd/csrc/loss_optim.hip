// Scalar losses (mean reduction) fused with their gradient, flat-buffer optimizers and the
// global gradient-norm clip.  All HBM-bound streaming kernels.
#include "srk_common.h"

namespace srk {

constexpr int kMaxPartials = 1024;  // doubles

// ---------------------------------------------------------------------------------------------
// Loss forward + backward in one pass.
//   pred/dpred : NHWC dense, element e = ((n*H+h)*W+w)*C + c
//   target     : element strides (sn, sc, sh, sw); `contig` = target is NHWC dense too.
// ---------------------------------------------------------------------------------------------
// a * b + c in two roundings whatever the context.  Left to the compiler's contraction, whether an expression becomes an fma
// depends on what else the optimizer finds next to it (a packed multiply takes the product away), so the 4-byte and the
// 16-byte form of one source line could round differently; the operations below are pinned to what both forms have
// always computed.
__device__ __forceinline__ float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
  return a * b + c;
}

// Exponential moving average of a parameter, from the value the optimizer has just computed (still in a register):
// ema + (1 - d) * (p - ema), a subtraction, a multiply and an add in fp32, three roundings whatever the context (see
// mul_then_add).
__device__ __forceinline__ float ema_update(float ema, float p_new, float one_minus_d) {
#pragma clang fp contract(off)
  const float diff = p_new - ema;
  return ema + one_minus_d * diff;
}
// The optional last argument of k_sgd / k_adam.  The kernels take it as a parameter pack: without it the kernel has the
// argument block, and the machine code, it had before there was an EMA (profiles/ema_asm.txt).
struct EmaArg {
  float* ema;
  float one_minus_d;   // 1.f - ema_decay, rounded once on the host
};
__host__ __device__ __forceinline__ EmaArg ema_of() { return {nullptr, 0.f}; }
__host__ __device__ __forceinline__ EmaArg ema_of(EmaArg a) { return a; }

__device__ __forceinline__ void loss_term(int kind, float p, float t, float eps, float& val, float& grad) {
  const float d = p - t;
  switch (kind) {
    case SRK_LOSS_MSE:
      val = d * d;
      grad = 2.f * d;
      break;
    case SRK_LOSS_L1:
      val = fabsf(d);
      grad = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      break;
    case SRK_LOSS_CHARBONNIER: {
      const float e = sqrtf(__builtin_fmaf(d, d, eps));  // lapsrn.py:81-85 (the fma spelled out: see mul_then_add)
      val = e;
      grad = d / e;
      break;
    }
    default: {  // BCE, torch semantics: logs clamped at -100, grad denominator clamped at 1e-12
      const float lp = fmaxf(logf(p), -100.f);
      const float l1p = fmaxf(logf(1.f - p), -100.f);
      val = -(t * lp + (1.f - t) * l1p);
      grad = (p - t) / fmaxf((1.f - p) * p, 1e-12f);
    }
  }
}

// One float (V = 1) or four (V = 4: dense, aligned tensors, pred, target and dpred in one layout) per thread and pass.  Each
// form keeps its own summation order: a thread adds its elements in lane order into one float, so the 16-byte form's
// partials are those of 4-element groups.  Only the 4-byte form walks a strided target.
template <int V>
__global__ __launch_bounds__(256) void k_loss_partial(int kind, const float* __restrict__ pred,
                                                      const float* __restrict__ target, int64_t sn, int64_t sc,
                                                      int64_t sh, int64_t sw, int contig, int C, int H, int W,
                                                      size_t groups, float eps, float gscale,
                                                      float* __restrict__ dpred, double* __restrict__ partials) {
  typedef Vec<V> Q;
  __shared__ double sm[4];
  float acc = 0.f;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < groups; e += (size_t)gridDim.x * 256) {
    size_t ti = e;
    if constexpr (V == 1) {
      if (!contig) {
        const int c = (int)(e % C);
        size_t t = e / C;
        const int w = (int)(t % W);
        t /= W;
        const int h = (int)(t % H);
        const size_t n = t / H;
        ti = n * sn + c * sc + h * sh + w * sw;
      }
    }
    const typename Q::T p = Q::load(pred, e), t = Q::load(target, ti);
    typename Q::T g;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float v, gg;
      loss_term(kind, Q::at(p, k), Q::at(t, k), eps, v, gg);
      acc += v;
      Q::set(g, k, gg * gscale);
    }
    if (dpred) Q::store(dpred, e, g);
  }
  store_block_sum_256_d((double)acc, sm, partials + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_loss_final(const double* __restrict__ partials, int nparts, double inv_count,
                                                    float* __restrict__ loss) {
  __shared__ double sm[4];
  const double tot = sum_partials_256_d(partials, nparts, sm);
  if (threadIdx.x == 0) *loss = (float)(tot * inv_count);
}

// ---------------------------------------------------------------------------------------------
// Optimizers.  V = 4 (n % 4 == 0, aligned buffers): the same operations per element, four elements per thread and pass
// (SRGAN-D's 23 M parameters under SGD: 184 -> ~100 us; the 4-byte loop moved 2.5 TB/s).
// EMA (srk_sgd_step_ema / srk_adam_step_ema): the shadow weights `ema` are updated from the new parameter value in the
// same pass, 8 more bytes per parameter and no launch of their own.  A compile-time switch (EMA, on when the kernel is
// instantiated with an EmaArg): off, the kernel is the one srk_sgd_step / srk_adam_step have always launched.
// ---------------------------------------------------------------------------------------------
template <int V, typename... Ema>
__global__ __launch_bounds__(256) void k_sgd(float* __restrict__ p, const float* __restrict__ g,
                                             float* __restrict__ buf, size_t groups, float lr, float mom, float wd,
                                             int nesterov, int first, const float* __restrict__ lr_dev,
                                             const float* __restrict__ gs_dev, Ema... ema_arg) {
  typedef Vec<V> Q;
  constexpr bool EMA = sizeof...(Ema) != 0;
  const EmaArg ea = ema_of(ema_arg...);
  if (lr_dev) lr = *lr_dev;
  const float gs = gs_dev ? *gs_dev : 1.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (size_t)gridDim.x * 256) {
    typename Q::T pi = Q::load(p, i);
    const typename Q::T gi = Q::load(g, i);
    typename Q::T bi = {};
    if (mom != 0.f && !first) bi = Q::load(buf, i);   // (the first step must not read the buffer)
    typename Q::T ei = {};
    if constexpr (EMA) ei = Q::load(ea.ema, i);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float d = Q::at(gi, e) * gs;
      if (wd != 0.f) d = mul_then_add(wd, Q::at(pi, e), d);   // (torch: grad.add(param, alpha = wd), a multiply and an add)
      if (mom != 0.f) {
        const float b = first ? d : Q::at(bi, e) * mom + d;
        Q::set(bi, e, b);
        d = nesterov ? d + mom * b : b;
      }
      Q::set(pi, e, Q::at(pi, e) - lr * d);
      if constexpr (EMA) Q::set(ei, e, ema_update(Q::at(ei, e), Q::at(pi, e), ea.one_minus_d));
    }
    if (mom != 0.f) Q::store(buf, i, bi);
    Q::store(p, i, pi);
    if constexpr (EMA) Q::store(ea.ema, i, ei);
  }
}

// Adam's step counter is advanced by the kernel itself (it used to be a one-thread launch of its own in front, ~5 us of a
// 1.2 ms train step): every block reads the count of the PREVIOUS steps before anything else (adam_begin) and works with
// count + 1; the block that finishes last -- a ticket in step_dev[1]: it has seen every other block's arrival, so every
// block has read the old count -- stores count + 1 and clears the ticket (adam_arrive).  The count is consumed by the
// next launch only.
struct AdamStep {
  int32_t count;            // this step's number, 1-based
  float step_size, bc2_sqrt;
};
__device__ __forceinline__ AdamStep adam_begin(const int32_t* __restrict__ step_dev, float lr, float b1, float b2) {
  AdamStep a;
  a.count = __hip_atomic_load(step_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
  const float t = (float)a.count;
  // torch/optim/adam.py (_single_tensor_adam): bias corrections, step_size, denom
  const float bc1 = 1.f - powf(b1, t);
  const float bc2 = 1.f - powf(b2, t);
  a.step_size = lr / bc1;
  a.bc2_sqrt = sqrtf(bc2);
  return a;
}
__device__ __forceinline__ void adam_arrive(int32_t* __restrict__ step_dev, int32_t count) {
  __syncthreads();   // (the whole block has read the old count)
  if (threadIdx.x == 0) {
    const int32_t arrived = atomicAdd(step_dev + 1, 1);
    if (arrived == (int32_t)gridDim.x - 1) {
      __hip_atomic_store(step_dev, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(step_dev + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The 16-byte form runs at most two blocks per CU (srk_adam_step): the arrival ticket is one atomic per block on one
// word, and ~740 of them in the 4-byte form's grid made the folded step counter cost what the separate launch had
// (EDSR: 19.4 vs 14.5 + 2.8 us).
template <int V, typename... Ema>
__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g,
                                              float* __restrict__ m, float* __restrict__ v, size_t groups, float lr,
                                              float b1, float b2, float eps, float wd,
                                              int32_t* __restrict__ step_dev, const float* __restrict__ lr_dev,
                                              const float* __restrict__ gs_dev, Ema... ema_arg) {
  typedef Vec<V> Q;
  constexpr bool EMA = sizeof...(Ema) != 0;
  const EmaArg ea = ema_of(ema_arg...);
  if (lr_dev) lr = *lr_dev;
  const float gs = gs_dev ? *gs_dev : 1.f;
  const AdamStep st = adam_begin(step_dev, lr, b1, b2);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (size_t)gridDim.x * 256) {
    typename Q::T pi = Q::load(p, i);
    const typename Q::T gv = Q::load(g, i);
    typename Q::T mi = Q::load(m, i), vi = Q::load(v, i);
    typename Q::T ei = {};
    if constexpr (EMA) ei = Q::load(ea.ema, i);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float gi = Q::at(gv, e) * gs;
      if (wd != 0.f) gi += wd * Q::at(pi, e);
      const float me = Q::at(mi, e) + (1.f - b1) * (gi - Q::at(mi, e));   // exp_avg.lerp_(grad, 1 - beta1)
      const float ve = Q::at(vi, e) * b2 + (1.f - b2) * gi * gi;
      Q::set(mi, e, me);
      Q::set(vi, e, ve);
      const float denom = sqrtf(ve) / st.bc2_sqrt + eps;
      Q::set(pi, e, Q::at(pi, e) - st.step_size * (me / denom));
      if constexpr (EMA) Q::set(ei, e, ema_update(Q::at(ei, e), Q::at(pi, e), ea.one_minus_d));
    }
    Q::store(m, i, mi);
    Q::store(v, i, vi);
    Q::store(p, i, pi);
    if constexpr (EMA) Q::store(ea.ema, i, ei);
  }
  adam_arrive(step_dev, st.count);
}

__global__ __launch_bounds__(256) void k_sqsum_partial(const float* __restrict__ g, size_t n,
                                                       double* __restrict__ partials) {
  __shared__ double sm[4];
  float acc = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float x = g[i];
    acc += x * x;
  }
  store_block_sum_256_d((double)acc, sm, partials + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_norm_final(const double* __restrict__ partials, int nparts, float max_norm,
                                                    float* __restrict__ norm_out, float* __restrict__ scale_out) {
  __shared__ double sm[4];
  const double tot = sum_partials_256_d(partials, nparts, sm);
  if (threadIdx.x == 0) {
    const float nrm = (float)sqrt(tot);
    if (norm_out) *norm_out = nrm;
    if (scale_out) {
      const float c = max_norm / (nrm + 1e-6f);  // torch.nn.utils.clip_grad_norm_
      *scale_out = c < 1.f ? c : 1.f;
    }
  }
}

}  // namespace srk

using namespace srk;

extern "C" size_t srk_loss_workspace_bytes(void) { return kMaxPartials * sizeof(double); }
extern "C" size_t srk_grad_norm_workspace_bytes(void) { return kMaxPartials * sizeof(double); }

extern "C" int srk_loss_forward_backward(int kind, const float* pred, const float* target,
                                         const int64_t* target_strides, int N, int C, int H, int W, float eps,
                                         float grad_scale, float* loss, float* dpred, void* workspace, void* stream) {
  SRK_REQUIRE(pred && target && loss && workspace, "loss: null pointer");
  SRK_REQUIRE(kind >= SRK_LOSS_MSE && kind <= SRK_LOSS_BCE, "loss: unknown kind %d", kind);
  SRK_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "loss: bad dims");
  const size_t total = (size_t)N * C * H * W;
  int64_t sn = (int64_t)H * W * C, sc = 1, sh = (int64_t)W * C, sw = C;
  int contig = 1;
  if (target_strides) {
    contig = (target_strides[0] == sn || N == 1) && (target_strides[1] == sc || C == 1) &&
             (target_strides[2] == sh || H == 1) && (target_strides[3] == sw || W == 1);
    sn = target_strides[0]; sc = target_strides[1]; sh = target_strides[2]; sw = target_strides[3];
  }
  hipStream_t s = (hipStream_t)stream;
  const bool vec = contig && (total & 3) == 0 && aligned16(pred, target, dpred);
  const size_t groups = vec ? total / 4 : total;
  const unsigned nb = vec ? grid_for(groups, 256, kMaxPartials) : grid_for(groups, 256 * 8, kMaxPartials);
  hipLaunchKernelGGL(vec ? k_loss_partial<4> : k_loss_partial<1>, dim3(nb), dim3(256), 0, s, kind, pred, target, sn, sc,
                     sh, sw, contig, C, H, W, groups, eps, grad_scale / (float)total, dpred, (double*)workspace);
  hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(256), 0, s, (const double*)workspace, (int)nb, 1.0 / (double)total,
                     loss);
  return check_launch("loss_forward_backward");
}

// One launcher per optimizer for the plain and the EMA entry point: the same form rule and the same grid.
template <bool EMA>
static int sgd_launch(float* p, const float* g, float* momentum_buf, size_t n, float lr, float momentum,
                      float weight_decay, int nesterov, int first_step, const float* lr_dev,
                      const float* grad_scale_dev, float* ema, float ema_decay, void* stream) {
  SRK_REQUIRE(p && g && n > 0, "sgd_step: null pointer or empty");
  SRK_REQUIRE(momentum == 0.f || momentum_buf, "sgd_step: momentum needs a buffer");
  const bool vec = (n & 3) == 0 && aligned16(p, g, momentum_buf, ema);
  const size_t groups = vec ? n / 4 : n;
  const unsigned nb = vec ? grid_for(groups, 256 * 2, 65535) : grid_for(groups, 256 * 8, kMaxPartials);   // two float4 / eight floats per thread
  if constexpr (EMA)
    hipLaunchKernelGGL((vec ? k_sgd<4, EmaArg> : k_sgd<1, EmaArg>), dim3(nb), dim3(256), 0, (hipStream_t)stream, p, g,
                       momentum_buf, groups, lr, momentum, weight_decay, nesterov, first_step, lr_dev, grad_scale_dev,
                       EmaArg{ema, 1.f - ema_decay});
  else
    hipLaunchKernelGGL(vec ? k_sgd<4> : k_sgd<1>, dim3(nb), dim3(256), 0, (hipStream_t)stream, p, g, momentum_buf,
                       groups, lr, momentum, weight_decay, nesterov, first_step, lr_dev, grad_scale_dev);
  return check_launch("sgd_step");
}

template <bool EMA>
static int adam_launch(float* p, const float* g, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int32_t* step_dev, const float* lr_dev,
                       const float* grad_scale_dev, float* ema, float ema_decay, void* stream) {
  SRK_REQUIRE(p && g && exp_avg && exp_avg_sq && step_dev && n > 0, "adam_step: null pointer or empty");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = n % 4 == 0 && aligned16(p, g, exp_avg, exp_avg_sq, ema);
  const size_t groups = vec ? n / 4 : n;
  const unsigned nb = vec ? grid_for(groups, 256 * 2, (size_t)2 * kNumCU) : grid_for(groups, 256 * 8, kMaxPartials);
  if constexpr (EMA)
    hipLaunchKernelGGL((vec ? k_adam<4, EmaArg> : k_adam<1, EmaArg>), dim3(nb), dim3(256), 0, s, p, g, exp_avg,
                       exp_avg_sq, groups, lr, beta1, beta2, eps, weight_decay, step_dev, lr_dev, grad_scale_dev,
                       EmaArg{ema, 1.f - ema_decay});
  else
    hipLaunchKernelGGL(vec ? k_adam<4> : k_adam<1>, dim3(nb), dim3(256), 0, s, p, g, exp_avg, exp_avg_sq, groups, lr,
                       beta1, beta2, eps, weight_decay, step_dev, lr_dev, grad_scale_dev);
  return check_launch("adam_step");
}

extern "C" int srk_sgd_step(float* p, const float* g, float* momentum_buf, size_t n, float lr, float momentum,
                            float weight_decay, int nesterov, int first_step, const float* lr_dev,
                            const float* grad_scale_dev, void* stream) {
  return sgd_launch<false>(p, g, momentum_buf, n, lr, momentum, weight_decay, nesterov, first_step, lr_dev,
                           grad_scale_dev, nullptr, 0.f, stream);
}

extern "C" int srk_sgd_step_ema(float* p, const float* g, float* momentum_buf, size_t n, float lr, float momentum,
                                float weight_decay, int nesterov, int first_step, const float* lr_dev,
                                const float* grad_scale_dev, float* ema, float ema_decay, void* stream) {
  SRK_REQUIRE(ema, "sgd_step_ema: null ema buffer");
  SRK_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, "sgd_step_ema: ema_decay %g outside [0, 1)", (double)ema_decay);
  return sgd_launch<true>(p, g, momentum_buf, n, lr, momentum, weight_decay, nesterov, first_step, lr_dev,
                          grad_scale_dev, ema, ema_decay, stream);
}

extern "C" int srk_adam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                             float beta1, float beta2, float eps, float weight_decay, int32_t* step_dev,
                             const float* lr_dev, const float* grad_scale_dev, void* stream) {
  return adam_launch<false>(p, g, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step_dev, lr_dev,
                            grad_scale_dev, nullptr, 0.f, stream);
}

extern "C" int srk_adam_step_ema(float* p, const float* g, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int32_t* step_dev,
                                 const float* lr_dev, const float* grad_scale_dev, float* ema, float ema_decay,
                                 void* stream) {
  SRK_REQUIRE(ema, "adam_step_ema: null ema buffer");
  SRK_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, "adam_step_ema: ema_decay %g outside [0, 1)", (double)ema_decay);
  return adam_launch<true>(p, g, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step_dev, lr_dev,
                           grad_scale_dev, ema, ema_decay, stream);
}

extern "C" int srk_grad_norm_clip(const float* g, size_t n, float max_norm, float* norm_out, float* scale_out,
                                  void* workspace, void* stream) {
  SRK_REQUIRE(g && workspace && n > 0, "grad_norm_clip: null pointer or empty");
  const unsigned nb = grid_for(n, 256 * 8, kMaxPartials);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sqsum_partial, dim3(nb), dim3(256), 0, s, g, n, (double*)workspace);
  hipLaunchKernelGGL(k_norm_final, dim3(1), dim3(256), 0, s, (const double*)workspace, (int)nb, max_norm, norm_out,
                     scale_out);
  return check_launch("grad_norm_clip");
}
