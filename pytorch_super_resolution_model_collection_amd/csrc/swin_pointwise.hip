// LayerNorm over the channel (last) axis with an affine, and the exact (erf) GELU: SwinIR's two pointwise operators.
// Definition: include/srk.h and DESIGN.md 29.  Kernels of their own: nothing here is a case of the elementwise or
// BatchNorm kernels, which stay as they are.
//
//   k_ln_fwd          one wave a row: mean, then the sum of squared differences (the row comes back from the cache), then
//                     y = (x - mean) * rstd * gamma + beta; mean and rstd are kept per row
//   k_ln_bwd_dx       one wave a row: sum(g dy) and sum(g dy xhat), then dx
//   k_ln_bwd_partial  one thread a column, one wave a range of rows: sum(dy xhat) and sum(dy) -> [ranges][2][C]
//   k_ln_bwd_finish   the ranges added up in a fixed order, in double, one wave an element
//   k_gelu_fwd / k_gelu_bwd<V>   16-byte accesses with a scalar tail where the pointers allow, else 4-byte
// No atomics: two calls give the same bits.
#include <math.h>

#include "srk_common.h"

namespace srk {

constexpr int kLnRowsPerRange = 16;
constexpr int kLnMaxRanges = 2048;

__global__ __launch_bounds__(256) void k_ln_fwd(const float* __restrict__ x, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, float* __restrict__ y,
                                                float* __restrict__ mean, float* __restrict__ rstd, int64_t rows, int C,
                                                float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  for (int64_t r = wave; r < rows; r += nwaves) {
    const float* xr = x + r * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += xr[c];
    const float mu = wave_sum(s) / (float)C;
    float v = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float dlt = xr[c] - mu;
      v = fmaf(dlt, dlt, v);
    }
    const float rs = 1.0f / sqrtf(wave_sum(v) / (float)C + eps);
    float* yr = y + r * C;
    for (int c = lane; c < C; c += 64) yr[c] = fmaf((xr[c] - mu) * rs, gamma[c], beta[c]);
    if (lane == 0 && mean) mean[r] = mu, rstd[r] = rs;
  }
}

// dx = rstd * (g dy - mean_c(g dy) - xhat * mean_c(g dy xhat))
__global__ __launch_bounds__(256) void k_ln_bwd_dx(const float* __restrict__ dy, const float* __restrict__ x,
                                                   const float* __restrict__ gamma, const float* __restrict__ mean,
                                                   const float* __restrict__ rstd, float* __restrict__ dx, int64_t rows,
                                                   int C) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  for (int64_t r = wave; r < rows; r += nwaves) {
    const float* xr = x + r * C;
    const float* gr = dy + r * C;
    const float mu = mean[r], rs = rstd[r];
    float a = 0.f, b = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float gd = gr[c] * gamma[c];
      a += gd;
      b = fmaf(gd, (xr[c] - mu) * rs, b);
    }
    a = wave_sum(a) / (float)C;
    b = wave_sum(b) / (float)C;
    float* dr = dx + r * C;
    for (int c = lane; c < C; c += 64) dr[c] = rs * (gr[c] * gamma[c] - a - (xr[c] - mu) * rs * b);
  }
}

// thread (column c, range k): rows [k * per, (k + 1) * per)
__global__ __launch_bounds__(256) void k_ln_bwd_partial(const float* __restrict__ dy, const float* __restrict__ x,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        float* __restrict__ partials, int64_t rows, int C, int ranges,
                                                        int64_t per) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (c >= C || k >= ranges) return;
  const int64_t r0 = (int64_t)k * per, r1 = r0 + per < rows ? r0 + per : rows;
  float dg = 0.f, db = 0.f;
#pragma unroll 4
  for (int64_t r = r0; r < r1; ++r) {
    const float g = dy[r * C + c];
    dg = fmaf(g, (x[r * C + c] - mean[r]) * rstd[r], dg);
    db += g;
  }
  partials[((size_t)k * 2) * C + c] = dg;
  partials[((size_t)k * 2 + 1) * C + c] = db;
}

__global__ __launch_bounds__(256) void k_ln_bwd_finish(const float* __restrict__ partials, float* __restrict__ dgamma,
                                                       float* __restrict__ dbeta, float acc, int C, int ranges) {
  // one wave an element: lane l adds ranges l, l + 64, ... in order, then the lanes are added in a fixed tree
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= 2 * C) return;
  const int which = i / C, c = i - which * C;
  float* out = which ? dbeta : dgamma;
  if (!out) return;
  double a = 0.0;
  for (int k = lane; k < ranges; k += 64) a += (double)partials[((size_t)k * 2 + which) * C + c];
  a = wave_sum_d(a);
  if (lane == 0) out[c] = acc == 0.f ? (float)a : acc * out[c] + (float)a;
}

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
// d/dx = Phi(x) + x phi(x)
__device__ __forceinline__ float gelu_df(float x) {
  return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * 0.39894228040143267794f * expf(-0.5f * x * x);
}

template <int V>
__global__ __launch_bounds__(256) void k_gelu_fwd(const float* __restrict__ x, float* __restrict__ y, size_t n) {
  const size_t nv = n / V, step = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += step) {
    typename Vec<V>::T v = Vec<V>::load(x, i);
#pragma unroll
    for (int e = 0; e < V; ++e) Vec<V>::set(v, e, gelu_f(Vec<V>::at(v, e)));
    Vec<V>::store(y, i, v);
  }
  if (blockIdx.x == 0)   // the scalar tail
    for (size_t i = nv * V + threadIdx.x; i < n; i += 256) y[i] = gelu_f(x[i]);
}

template <int V>
__global__ __launch_bounds__(256) void k_gelu_bwd(const float* __restrict__ dy, const float* __restrict__ x,
                                                  float* __restrict__ dx, size_t n) {
  const size_t nv = n / V, step = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += step) {
    const typename Vec<V>::T v = Vec<V>::load(x, i), g = Vec<V>::load(dy, i);
    typename Vec<V>::T o;
#pragma unroll
    for (int e = 0; e < V; ++e) Vec<V>::set(o, e, Vec<V>::at(g, e) * gelu_df(Vec<V>::at(v, e)));
    Vec<V>::store(dx, i, o);
  }
  if (blockIdx.x == 0)
    for (size_t i = nv * V + threadIdx.x; i < n; i += 256) dx[i] = dy[i] * gelu_df(x[i]);
}

static int ln_ranges(int64_t rows) {
  const int64_t k = (rows + kLnRowsPerRange - 1) / kLnRowsPerRange;
  return (int)(k < kLnMaxRanges ? k : kLnMaxRanges);
}

}  // namespace srk

using namespace srk;

extern "C" size_t srk_layer_norm_workspace(int64_t rows, int C) {
  if (rows <= 0 || C <= 0) return 0;
  return (size_t)ln_ranges(rows) * 2 * C * sizeof(float);
}

extern "C" int srk_layer_norm_forward(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                                      float* rstd, int64_t rows, int C, float eps, void* stream) {
  const char* who = "layer_norm_forward";
  SRK_REQUIRE(x && gamma && beta && y, "%s: null pointer", who);
  SRK_REQUIRE((mean && rstd) || (!mean && !rstd), "%s: mean and rstd are saved together or not at all", who);
  SRK_REQUIRE(rows > 0 && C > 0, "%s: bad dims (rows %lld, C %d)", who, (long long)rows, C);
  hipLaunchKernelGGL(k_ln_fwd, dim3(grid_for((size_t)rows, 4, (size_t)kNumCU * 8)), dim3(256), 0, (hipStream_t)stream, x,
                     gamma, beta, y, mean, rstd, rows, C, eps);
  return check_launch(who);
}

extern "C" int srk_layer_norm_backward(const float* dy, const float* x, const float* gamma, const float* mean,
                                       const float* rstd, float* dx, float* dgamma, float* dbeta, float acc, int64_t rows,
                                       int C, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "layer_norm_backward";
  SRK_REQUIRE(dy && x && gamma && mean && rstd, "%s: null pointer", who);
  SRK_REQUIRE(dx || dgamma || dbeta, "%s: nothing to compute", who);
  SRK_REQUIRE(rows > 0 && C > 0, "%s: bad dims (rows %lld, C %d)", who, (long long)rows, C);
  if (dgamma || dbeta) {   // (refused before anything is launched)
    SRK_REQUIRE(workspace, "%s: null pointer (the parameter gradients need the workspace)", who);
    if (workspace_bytes < srk_layer_norm_workspace(rows, C)) {
      set_error("%s: workspace of %zu bytes, srk_layer_norm_workspace says %zu", who, workspace_bytes,
                srk_layer_norm_workspace(rows, C));
      return SRK_ERR_WORKSPACE;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  if (dx)
    hipLaunchKernelGGL(k_ln_bwd_dx, dim3(grid_for((size_t)rows, 4, (size_t)kNumCU * 8)), dim3(256), 0, st, dy, x, gamma,
                       mean, rstd, dx, rows, C);
  if (dgamma || dbeta) {
    const int ranges = ln_ranges(rows);
    const int64_t per = (rows + ranges - 1) / ranges;
    hipLaunchKernelGGL(k_ln_bwd_partial, dim3(cdiv((size_t)C, 64), cdiv((size_t)ranges, 4)), dim3(256), 0, st, dy, x, mean,
                       rstd, (float*)workspace, rows, C, ranges, per);
    hipLaunchKernelGGL(k_ln_bwd_finish, dim3(cdiv((size_t)2 * C, 4)), dim3(256), 0, st, (const float*)workspace, dgamma,
                       dbeta, acc, C, ranges);
  }
  return check_launch(who);
}

extern "C" int srk_gelu_forward(const float* x, float* y, size_t n, void* stream) {
  const char* who = "gelu_forward";
  SRK_REQUIRE(x && y, "%s: null pointer", who);
  SRK_REQUIRE(n > 0, "%s: empty tensor", who);
  hipStream_t st = (hipStream_t)stream;
  if (aligned16(x, y))
    hipLaunchKernelGGL(k_gelu_fwd<4>, dim3(grid_for(n / 4, 1024, (size_t)kNumCU * 8)), dim3(256), 0, st, x, y, n);
  else
    hipLaunchKernelGGL(k_gelu_fwd<1>, dim3(grid_for(n, 1024, (size_t)kNumCU * 8)), dim3(256), 0, st, x, y, n);
  return check_launch(who);
}

extern "C" int srk_gelu_backward(const float* dy, const float* x, float* dx, size_t n, void* stream) {
  const char* who = "gelu_backward";
  SRK_REQUIRE(dy && x && dx, "%s: null pointer", who);
  SRK_REQUIRE(n > 0, "%s: empty tensor", who);
  hipStream_t st = (hipStream_t)stream;
  if (aligned16(dy, x, dx))
    hipLaunchKernelGGL(k_gelu_bwd<4>, dim3(grid_for(n / 4, 1024, (size_t)kNumCU * 8)), dim3(256), 0, st, dy, x, dx, n);
  else
    hipLaunchKernelGGL(k_gelu_bwd<1>, dim3(grid_for(n, 1024, (size_t)kNumCU * 8)), dim3(256), 0, st, dy, x, dx, n);
  return check_launch(who);
}
