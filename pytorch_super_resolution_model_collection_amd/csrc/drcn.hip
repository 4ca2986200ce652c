// DRCN's recursive-supervision head (drcn.py:38-52, 200-215): the weighted combine of the D reconstructions
//   out = x + (sum_d w_d * Y_d) / sum_d w_d
// for inference, and for training the loss
//   L = a * mean_d MSE(Y_d, t) + (1 - a) * MSE(out, t) + b*R
// with its gradients to every Y_d and to w, produced in the same pass (seed folded in, as srk_loss_forward_backward does).
// Every kernel here streams: one read of each Y_d, x and t, one write of out and of every dY_d.  The sums go through
// per-block partial slabs and a one-block finalize in a fixed order (no float atomics: bit-equal on every run).
#include "srk_common.h"

namespace srk {

constexpr int kDrcnMaxBlocks = 1024;

// sum_d w_d in the reference's order (the same value in every thread: w is read through the scalar cache)
__device__ __forceinline__ float drcn_wsum(const float* __restrict__ w, int D) {
  float s = 0.f;
  for (int d = 0; d < D; ++d) s += w[d];
  return s;
}

// ---- inference combine: out = x + (sum_d w_d Y_d) * (1 / sum w) ------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void k_drcn_combine(const float* __restrict__ Y, const float* __restrict__ x,
                                                      const float* __restrict__ w, int D, size_t M, size_t groups,
                                                      float* __restrict__ out) {
  typedef Vec<V> Q;
  const float inv_s = 1.f / drcn_wsum(w, D);
  const size_t Mg = M / V;   // Y_d is the d-th block of M elements
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
    typename Q::T acc = Q::load(Y, g) * w[0];
    for (int d = 1; d < D; ++d) acc = acc + Q::load(Y, (size_t)d * Mg + g) * w[d];
    Q::store(out, g, Q::load(x, g) + acc * inv_s);
  }
}

// ---- training: out, every dY_d and the per-block partial sums in one pass ------------------------------------------
// partials (doubles): [q][block], q = 0: sum (Y_d - t)^2 over d and elements, 1: sum (out - t)^2, 2 + d: sum g*(Y_d - c)
// DM: compile-time bound of D (the D values of an element group stay in registers); V: elements per thread and pass.
template <int DM, int V>
__global__ __launch_bounds__(256) void k_drcn_loss(const float* __restrict__ Y, const float* __restrict__ x,
                                                   const float* __restrict__ t, const float* __restrict__ w, int D,
                                                   size_t M, size_t groups, const float* __restrict__ alpha_dev,
                                                   float grad_scale, float* __restrict__ out, float* __restrict__ dY,
                                                   double* __restrict__ partials) {
  typedef Vec<V> Q;
  __shared__ double sm[DM + 2][4];
  const float S = drcn_wsum(w, D);
  const float inv_s = 1.f / S;
  const float alpha = *alpha_dev;
  const float k_out = grad_scale * (1.f - alpha) * 2.f / (float)M;       // d(1-a)MSE(out)/d out   per (out - t)
  const float k_y = grad_scale * alpha * 2.f / ((float)D * (float)M);    // d a mean_d MSE_d/d Y_d per (Y_d - t)
  float wd[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) wd[d] = d < D ? w[d] : 0.f;
  float l1 = 0.f, l2 = 0.f, pw[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) pw[d] = 0.f;
  const size_t Mg = M / V;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
    typename Q::T y[DM];
#pragma unroll
    for (int d = 0; d < DM; ++d)
      if (d < D) y[d] = Q::load(Y, (size_t)d * Mg + g);
    const typename Q::T xv = Q::load(x, g), tv = Q::load(t, g);
    typename Q::T ov;
    float gk[V], ck[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float acc = Q::at(y[0], k) * wd[0];
#pragma unroll
      for (int d = 1; d < DM; ++d)
        if (d < D) acc += Q::at(y[d], k) * wd[d];
      const float c = acc * inv_s;
      const float o = Q::at(xv, k) + c;
      const float eo = o - Q::at(tv, k);
      l2 += eo * eo;
      Q::set(ov, k, o);
      gk[k] = k_out * eo;
      ck[k] = c;
    }
    Q::store(out, g, ov);
#pragma unroll
    for (int d = 0; d < DM; ++d) {
      if (d < D) {
        typename Q::T dy;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float yv = Q::at(y[d], k);
          const float e = yv - Q::at(tv, k);
          l1 += e * e;
          pw[d] += gk[k] * (yv - ck[k]);
          Q::set(dy, k, k_y * e + gk[k] * wd[d] * inv_s);
        }
        Q::store(dY, (size_t)d * Mg + g, dy);
      }
    }
  }
  // block partials: every wave reduces its D + 2 sums, one pass over the four waves' values
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double r = wave_sum_d((double)l1);
  if (lane == 0) sm[0][wv] = r;
  r = wave_sum_d((double)l2);
  if (lane == 0) sm[1][wv] = r;
#pragma unroll
  for (int d = 0; d < DM; ++d) {
    if (d < D) {
      r = wave_sum_d((double)pw[d]);
      if (lane == 0) sm[2 + d][wv] = r;
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < D + 2; q += 256)
    partials[(size_t)q * gridDim.x + blockIdx.x] = sm[q][0] + sm[q][1] + sm[q][2] + sm[q][3];
}

// ---- backward of the combine for an arbitrary upstream gradient g of out (a loss the caller composes itself) ---------
//   dY_d = g * w_d / sum w,  partial slabs of sum g*(Y_d - c) with c recomputed as the forward combine computes it
// partials: the loss kernel's layout (q = 0, 1 written as 0: k_drcn_final finishes both kernels)
template <int DM, int V>
__global__ __launch_bounds__(256) void k_drcn_combine_bwd(const float* __restrict__ Y, const float* __restrict__ gout,
                                                          const float* __restrict__ w, int D, size_t M, size_t groups,
                                                          float* __restrict__ dY, double* __restrict__ partials) {
  typedef Vec<V> Q;
  __shared__ double sm[DM][4];
  const float inv_s = 1.f / drcn_wsum(w, D);
  float wd[DM], pw[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) {
    wd[d] = d < D ? w[d] : 0.f;
    pw[d] = 0.f;
  }
  const size_t Mg = M / V;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
    typename Q::T y[DM];
#pragma unroll
    for (int d = 0; d < DM; ++d)
      if (d < D) y[d] = Q::load(Y, (size_t)d * Mg + g);
    const typename Q::T gv = Q::load(gout, g);
    float ck[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float acc = Q::at(y[0], k) * wd[0];
#pragma unroll
      for (int d = 1; d < DM; ++d)
        if (d < D) acc = acc + Q::at(y[d], k) * wd[d];
      ck[k] = acc * inv_s;
    }
#pragma unroll
    for (int d = 0; d < DM; ++d) {
      if (d < D) {
        typename Q::T dy;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float gk = Q::at(gv, k);
          pw[d] += gk * (Q::at(y[d], k) - ck[k]);
          Q::set(dy, k, gk * wd[d] * inv_s);
        }
        Q::store(dY, (size_t)d * Mg + g, dy);
      }
    }
  }
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 0; d < DM; ++d) {
    if (d < D) {
      const double r = wave_sum_d((double)pw[d]);
      if (lane == 0) sm[d][wv] = r;
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < D + 2; q += 256)
    partials[(size_t)q * gridDim.x + blockIdx.x] =
        q < 2 ? 0.0 : sm[q - 2][0] + sm[q - 2][1] + sm[q - 2][2] + sm[q - 2][3];
}

// one block: the scalar loss (and its two MSE terms), dw = beta * dw + (sum g*(Y_d - c)) / sum w
__global__ __launch_bounds__(256) void k_drcn_final(const double* __restrict__ partials, int nparts, int D, size_t M,
                                                    const float* __restrict__ w, const float* __restrict__ alpha_dev,
                                                    const float* __restrict__ reg_dev, float* __restrict__ loss,
                                                    float* __restrict__ terms, float* __restrict__ dw, float dw_beta) {
  __shared__ double sm[4];
  __shared__ double s01[2];
  const float S = drcn_wsum(w, D);
  for (int q = 0; q < D + 2; ++q) {
    const double tot = sum_partials_256_d(partials + (size_t)q * nparts, nparts, sm);
    if (threadIdx.x == 0) {
      if (q < 2) {
        s01[q] = tot;
      } else if (dw) {
        const float v = (float)(tot / (double)S);
        dw[q - 2] = dw_beta == 0.f ? v : dw_beta * dw[q - 2] + v;
      }
    }
  }
  if (threadIdx.x == 0) {
    const double l1 = s01[0] / ((double)D * (double)M), l2 = s01[1] / (double)M;
    const double a = alpha_dev ? (double)*alpha_dev : 0.0;
    const double r = reg_dev ? (double)*reg_dev : 0.0;
    if (loss) *loss = (float)(a * l1 + (1.0 - a) * l2 + r);
    if (terms) {
      terms[0] = (float)l1;
      terms[1] = (float)l2;
    }
  }
}

// ---- sum of squares of a flat buffer (the weight-decay term R of drcn.py:212-214), fp64 per thread ----------------
template <int V>
__global__ __launch_bounds__(256) void k_sumsq_partial(const float* __restrict__ p, size_t groups,
                                                       double* __restrict__ partials) {
  typedef Vec<V> Q;
  __shared__ double sm[4];
  double acc = 0.0;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
    const typename Q::T v = Q::load(p, g);
#pragma unroll
    for (int k = 0; k < V; ++k) acc += (double)Q::at(v, k) * (double)Q::at(v, k);
  }
  store_block_sum_256_d(acc, sm, partials + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_sumsq_final(const double* __restrict__ partials, int nparts, float scale,
                                                     float* __restrict__ out) {
  __shared__ double sm[4];
  const double tot = sum_partials_256_d(partials, nparts, sm);
  if (threadIdx.x == 0) *out = (float)((double)scale * tot);
}

}  // namespace srk

using namespace srk;

extern "C" size_t srk_drcn_workspace_bytes(int D) {
  return D < 1 ? 0 : (size_t)(D + 2) * kDrcnMaxBlocks * sizeof(double);
}

extern "C" int srk_drcn_head_forward(const float* Y, const float* x, const float* w, int D, int N, int C, int H, int W,
                                     float* out, void* stream) {
  SRK_REQUIRE(Y && x && w && out, "drcn_head_forward: null pointer");
  SRK_REQUIRE(D >= 1 && D <= SRK_DRCN_MAX_D, "drcn_head_forward: D = %d outside [1, %d]", D, SRK_DRCN_MAX_D);
  SRK_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "drcn_head_forward: bad dims");
  const size_t M = (size_t)N * C * H * W;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = M % 4 == 0 && aligned16(Y, x, out);
  const size_t groups = vec ? M / 4 : M;
  hipLaunchKernelGGL(vec ? k_drcn_combine<4> : k_drcn_combine<1>, dim3(grid_for(groups, 256, kDrcnMaxBlocks)),
                     dim3(256), 0, s, Y, x, w, D, M, groups, out);
  return check_launch("drcn_head_forward");
}

extern "C" int srk_drcn_head_loss(const float* Y, const float* x, const float* target, const float* w, int D, int N,
                                  int C, int H, int W, const float* alpha_dev, const float* reg_dev, float grad_scale,
                                  float* out, float* dY, float* loss, float* terms, float* dw, float dw_beta,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  SRK_REQUIRE(Y && x && target && w && alpha_dev && out && dY && loss && workspace, "drcn_head_loss: null pointer");
  SRK_REQUIRE(D >= 1 && D <= SRK_DRCN_MAX_D, "drcn_head_loss: D = %d outside [1, %d]", D, SRK_DRCN_MAX_D);
  SRK_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "drcn_head_loss: bad dims");
  SRK_REQUIRE(workspace_bytes >= srk_drcn_workspace_bytes(D), "drcn_head_loss: workspace of %zu bytes < %zu",
              workspace_bytes, srk_drcn_workspace_bytes(D));
  const size_t M = (size_t)N * C * H * W;
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  const bool vec = M % 4 == 0 && aligned16(Y, x, target, out, dY);
  const size_t groups = vec ? M / 4 : M;
  const unsigned nb = grid_for(groups, 256, kDrcnMaxBlocks);
#define SRK_DRCN_LOSS(DM, V)                                                                                          \
  hipLaunchKernelGGL((k_drcn_loss<DM, V>), dim3(nb), dim3(256), 0, s, Y, x, target, w, D, M, groups, alpha_dev,      \
                     grad_scale, out, dY, part)
  if (vec) {
    if (D <= 4) SRK_DRCN_LOSS(4, 4);
    else if (D <= 16) SRK_DRCN_LOSS(16, 4);
    else SRK_DRCN_LOSS(32, 1);   // (32 D values of four elements would not stay in registers: the scalar form)
  } else {
    if (D <= 4) SRK_DRCN_LOSS(4, 1);
    else if (D <= 16) SRK_DRCN_LOSS(16, 1);
    else SRK_DRCN_LOSS(32, 1);
  }
#undef SRK_DRCN_LOSS
  hipLaunchKernelGGL(k_drcn_final, dim3(1), dim3(256), 0, s, (const double*)part, (int)nb, D, M, w, alpha_dev, reg_dev,
                     loss, terms, dw, dw_beta);
  return check_launch("drcn_head_loss");
}

extern "C" int srk_drcn_head_backward(const float* Y, const float* w, const float* dout, int D, int N, int C, int H,
                                      int W, float* dY, float* dw, float dw_beta, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  SRK_REQUIRE(Y && w && dout && dY && workspace, "drcn_head_backward: null pointer");
  SRK_REQUIRE(D >= 1 && D <= SRK_DRCN_MAX_D, "drcn_head_backward: D = %d outside [1, %d]", D, SRK_DRCN_MAX_D);
  SRK_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "drcn_head_backward: bad dims");
  SRK_REQUIRE(workspace_bytes >= srk_drcn_workspace_bytes(D), "drcn_head_backward: workspace of %zu bytes < %zu",
              workspace_bytes, srk_drcn_workspace_bytes(D));
  const size_t M = (size_t)N * C * H * W;
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  const bool vec = M % 4 == 0 && aligned16(Y, dout, dY);
  const size_t groups = vec ? M / 4 : M;
  const unsigned nb = grid_for(groups, 256, kDrcnMaxBlocks);
#define SRK_DRCN_BWD(DM, V)                                                                                           \
  hipLaunchKernelGGL((k_drcn_combine_bwd<DM, V>), dim3(nb), dim3(256), 0, s, Y, dout, w, D, M, groups, dY, part)
  if (vec) {
    if (D <= 4) SRK_DRCN_BWD(4, 4);
    else if (D <= 16) SRK_DRCN_BWD(16, 4);
    else SRK_DRCN_BWD(32, 1);
  } else {
    if (D <= 4) SRK_DRCN_BWD(4, 1);
    else if (D <= 16) SRK_DRCN_BWD(16, 1);
    else SRK_DRCN_BWD(32, 1);
  }
#undef SRK_DRCN_BWD
  if (dw)
    hipLaunchKernelGGL(k_drcn_final, dim3(1), dim3(256), 0, s, (const double*)part, (int)nb, D, M, w, nullptr, nullptr,
                       nullptr, nullptr, dw, dw_beta);
  return check_launch("drcn_head_backward");
}

extern "C" size_t srk_sumsq_workspace_bytes(void) { return kDrcnMaxBlocks * sizeof(double); }

extern "C" int srk_sumsq(const float* p, size_t n, float scale, float* out, void* workspace, void* stream) {
  SRK_REQUIRE(p && out && workspace && n > 0, "sumsq: null pointer or empty");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = n % 4 == 0 && aligned16(p);
  const size_t groups = vec ? n / 4 : n;
  const unsigned nb = grid_for(groups, 256, kDrcnMaxBlocks);
  hipLaunchKernelGGL(vec ? k_sumsq_partial<4> : k_sumsq_partial<1>, dim3(nb), dim3(256), 0, s, p, groups,
                     (double*)workspace);
  hipLaunchKernelGGL(k_sumsq_final, dim3(1), dim3(256), 0, s, (const double*)workspace, (int)nb, scale, out);
  return check_launch("sumsq");
}
