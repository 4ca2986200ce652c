// Channel attention (the gate of RCAN's residual channel attention block), forward and backward.  Definition:
// include/srk.h and DESIGN.md 25; the MLP is ca_common.h's, shared with the host twin.
//
//   forward    k_ca_colsum<V, false>   per-sample column sums of t over a range of pixels, fp64      -> [N][splits][C]
//              k_ca_gate_apply<V>      every block adds its sample's partials up again, runs the C -> Cr -> C MLP itself and
//                                      writes y = t * s (+ x) for its pixels; the sample's first block stores m, h and s
//   backward   k_ca_colsum<V, true>    the same sums of g * t
//              k_ca_bwd_apply<V>       finish, MLP backward, dt = g * s + dm / HW; the first block stores da and dh
//              k_ca_param_grads        dW1, db1, dW2, db2: one thread an element, the samples added in index order
// (the pattern of k_bn_fin_apply_act: the finish needs no launch and no hand-off if every block redoes it for itself).
// V = 4 floats an access where C % 4 == 0 and the tensors sit on 16-byte boundaries, else V = 1.  A thread keeps its
// column group for the whole pass (256 / (C / V) pixels go through a block at a time), so the column sums need no
// per-element index arithmetic and the gate is read into registers once.  No atomics: two calls give the same bits.
#include <math.h>

#include <vector>

#include "ca_common.h"
#include "srk_common.h"

namespace srk {

// threads of a block that stream: whole pixels only (C / V column groups each)
__device__ __forceinline__ int ca_active(int G) { return (256 / G) * G; }

// sum over pixels [r0, r1) of one sample of a (or a * b), per column -> partials[(n * splits + sp) * C + c]
template <int V, bool MUL>
__global__ __launch_bounds__(256) void k_ca_colsum(const float* __restrict__ a, const float* __restrict__ b,
                                                   double* __restrict__ partials, int64_t rows, int C, int splits) {
  __shared__ double red[256 * V];
  const int G = C / V, tid = threadIdx.x;
  const int n = blockIdx.x / splits, sp = blockIdx.x - n * splits;
  const int64_t per = (rows + splits - 1) / splits;
  const int64_t r0 = (int64_t)sp * per < rows ? (int64_t)sp * per : rows;
  const int64_t r1 = r0 + per < rows ? r0 + per : rows;
  const size_t base = (size_t)n * rows * C;   // in floats; a multiple of V
  const float* ap = a + base;
  const float* bp = MUL ? b + base : nullptr;
  double acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = 0.0;
  auto add = [&](const typename Vec<V>::T& va, const typename Vec<V>::T& vb) {
#pragma unroll
    for (int e = 0; e < V; ++e)
      acc[e] += MUL ? (double)Vec<V>::at(va, e) * (double)Vec<V>::at(vb, e) : (double)Vec<V>::at(va, e);
  };
  if (tid < ca_active(G)) {
    const size_t step = (size_t)ca_active(G), end = (size_t)r1 * G;
    size_t i = (size_t)r0 * G + tid;
    for (; i + 3 * step < end; i += 4 * step) {   // four loads in flight; added in the order of the plain loop
      typename Vec<V>::T va[4], vb[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        va[k] = Vec<V>::load(ap, i + k * step);
        vb[k] = MUL ? Vec<V>::load(bp, i + k * step) : va[k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) add(va[k], vb[k]);
    }
    for (; i < end; i += step) {
      const typename Vec<V>::T va = Vec<V>::load(ap, i);
      add(va, MUL ? Vec<V>::load(bp, i) : va);
    }
  }
  // thread tid = pixel lane * G + column group: red is [pixel lane][C]
#pragma unroll
  for (int e = 0; e < V; ++e) red[tid * V + e] = acc[e];
  __syncthreads();
  if (tid < C) {
    const int lanes = 256 / G;
    double s = 0.0;
    SRK_CA_UNROLL
    for (int l = 0; l < lanes; ++l) s += red[l * C + tid];
    partials[((size_t)n * splits + sp) * C + tid] = s;
  }
}

// the sample's column total, its partials added in index order
__device__ __forceinline__ double ca_finish(const double* __restrict__ partials, int n, int splits, int C, int c) {
  double s = 0.0;
  SRK_CA_UNROLL
  for (int k = 0; k < splits; ++k) s += partials[((size_t)n * splits + k) * C + c];
  return s;
}

struct CaGeom {
  int64_t rows;         // H * W
  int64_t apply_rows;   // pixels per block of the apply pass
  int C, Cr, splits, blocks_per_sample;
};

// y = t * s (+ x) over the block's pixels, s from the block's own finish and MLP
template <int V>
__global__ __launch_bounds__(256) void k_ca_gate_apply(const float* __restrict__ t, const float* __restrict__ x,
                                                       float* __restrict__ y, const double* __restrict__ partials,
                                                       const float* __restrict__ w1, const float* __restrict__ b1,
                                                       const float* __restrict__ w2, const float* __restrict__ b2,
                                                       float* __restrict__ save_m, float* __restrict__ save_h,
                                                       float* __restrict__ save_s, CaGeom q) {
  __shared__ double sm_m[kCaMaxC], sm_s[kCaMaxC], sm_h[kCaMaxCr];
  const int C = q.C, Cr = q.Cr, G = C / V, tid = threadIdx.x;
  const int n = blockIdx.x / q.blocks_per_sample, rb = blockIdx.x - n * q.blocks_per_sample;
  if (tid < C) sm_m[tid] = ca_finish(partials, n, q.splits, C, tid) / (double)q.rows;
  __syncthreads();
  if (tid < Cr) sm_h[tid] = ca_hidden(tid, sm_m, w1, b1, C);
  __syncthreads();
  if (tid < C) sm_s[tid] = ca_gate(tid, sm_h, w2, b2, Cr);
  __syncthreads();
  if (rb == 0 && save_s) {   // what the backward needs of this sample
    if (tid < C) save_m[(size_t)n * C + tid] = (float)sm_m[tid], save_s[(size_t)n * C + tid] = (float)sm_s[tid];
    if (tid < Cr) save_h[(size_t)n * Cr + tid] = (float)sm_h[tid];
  }
  if (tid >= ca_active(G)) return;
  typename Vec<V>::T sv;
#pragma unroll
  for (int e = 0; e < V; ++e) Vec<V>::set(sv, e, (float)sm_s[(tid % G) * V + e]);
  const size_t base = (size_t)n * q.rows * C;
  const float* tp = t + base;
  const float* xp = x ? x + base : nullptr;
  float* yp = y + base;
  const int64_t r0 = (int64_t)rb * q.apply_rows;
  const int64_t r1 = r0 + q.apply_rows < q.rows ? r0 + q.apply_rows : q.rows;
  const size_t step = (size_t)ca_active(G), end = (size_t)r1 * G;
  size_t i = (size_t)r0 * G + tid;
  for (; i + 3 * step < end; i += 4 * step) {
    typename Vec<V>::T tv[4], xv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      tv[k] = Vec<V>::load(tp, i + k * step);
      if (xp) xv[k] = Vec<V>::load(xp, i + k * step);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) Vec<V>::store(yp, i + k * step, xp ? tv[k] * sv + xv[k] : tv[k] * sv);
  }
  for (; i < end; i += step) {
    const typename Vec<V>::T tv = Vec<V>::load(tp, i);
    Vec<V>::store(yp, i, xp ? tv * sv + Vec<V>::load(xp, i) : tv * sv);
  }
}

// dt = g * s + dm / HW over the block's pixels; ds from the block's own finish of the g * t partials
template <int V>
__global__ __launch_bounds__(256) void k_ca_bwd_apply(const float* __restrict__ g, float* __restrict__ dt,
                                                      const double* __restrict__ partials, const float* __restrict__ w1,
                                                      const float* __restrict__ w2, const float* __restrict__ save_h,
                                                      const float* __restrict__ save_s, double* __restrict__ ws_da,
                                                      double* __restrict__ ws_dh, CaGeom q) {
  __shared__ double sm_da[kCaMaxC], sm_dm[kCaMaxC], sm_dh[kCaMaxCr];
  __shared__ float sm_s[kCaMaxC], sm_h[kCaMaxCr];
  const int C = q.C, Cr = q.Cr, G = C / V, tid = threadIdx.x;
  const int n = blockIdx.x / q.blocks_per_sample, rb = blockIdx.x - n * q.blocks_per_sample;
  if (tid < C) {
    const float s = save_s[(size_t)n * C + tid];
    sm_s[tid] = s;
    sm_da[tid] = ca_dgate(ca_finish(partials, n, q.splits, C, tid), (double)s);
  }
  if (tid < Cr) sm_h[tid] = save_h[(size_t)n * Cr + tid];
  __syncthreads();
  if (tid < Cr) sm_dh[tid] = ca_dhidden(tid, sm_da, w2, sm_h, C, Cr);
  __syncthreads();
  if (tid < C) sm_dm[tid] = ca_dmean(tid, sm_dh, w1, C, Cr) / (double)q.rows;
  __syncthreads();
  if (rb == 0) {   // what k_ca_param_grads needs of this sample
    if (tid < C) ws_da[(size_t)n * C + tid] = sm_da[tid];
    if (tid < Cr) ws_dh[(size_t)n * Cr + tid] = sm_dh[tid];
  }
  if (tid >= ca_active(G)) return;
  typename Vec<V>::T sv, dv;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    Vec<V>::set(sv, e, sm_s[(tid % G) * V + e]);
    Vec<V>::set(dv, e, (float)sm_dm[(tid % G) * V + e]);
  }
  const size_t base = (size_t)n * q.rows * C;
  const float* gp = g + base;
  float* dp = dt + base;
  const int64_t r0 = (int64_t)rb * q.apply_rows;
  const int64_t r1 = r0 + q.apply_rows < q.rows ? r0 + q.apply_rows : q.rows;
  const size_t step = (size_t)ca_active(G), end = (size_t)r1 * G;
  size_t i = (size_t)r0 * G + tid;
  for (; i + 3 * step < end; i += 4 * step) {
    typename Vec<V>::T gv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) gv[k] = Vec<V>::load(gp, i + k * step);
#pragma unroll
    for (int k = 0; k < 4; ++k) Vec<V>::store(dp, i + k * step, gv[k] * sv + dv);
  }
  for (; i < end; i += step) Vec<V>::store(dp, i, Vec<V>::load(gp, i) * sv + dv);
}

// The four parameter gradients, laid out one after the other: dW1 [Cr][C], dW2 [C][Cr], db1 [Cr], db2 [C].
// value(i) = the sum over the samples, in index order, of element i of that layout.
template <typename M, typename H>
__host__ __device__ __forceinline__ double ca_param_grad(int64_t i, const double* da, const double* dh, const M* m,
                                                         const H* h, int N, int C, int Cr) {
  const int64_t nw = (int64_t)C * Cr;
  double a = 0.0;
  if (i < nw) {   // dW1[j][c] = sum_n dh[n][j] * m[n][c]
    const int j = (int)(i / C), c = (int)(i - (int64_t)j * C);
    SRK_CA_UNROLL
    for (int n = 0; n < N; ++n) a = fma(dh[(size_t)n * Cr + j], (double)m[(size_t)n * C + c], a);
  } else if (i < 2 * nw) {   // dW2[c][j] = sum_n da[n][c] * h[n][j]
    const int c = (int)((i - nw) / Cr), j = (int)(i - nw - (int64_t)c * Cr);
    SRK_CA_UNROLL
    for (int n = 0; n < N; ++n) a = fma(da[(size_t)n * C + c], (double)h[(size_t)n * Cr + j], a);
  } else if (i < 2 * nw + Cr) {
    SRK_CA_UNROLL
    for (int n = 0; n < N; ++n) a += dh[(size_t)n * Cr + (i - 2 * nw)];
  } else {
    SRK_CA_UNROLL
    for (int n = 0; n < N; ++n) a += da[(size_t)n * C + (i - 2 * nw - Cr)];
  }
  return a;
}

__global__ __launch_bounds__(256) void k_ca_param_grads(const double* __restrict__ da, const double* __restrict__ dh,
                                                        const float* __restrict__ m, const float* __restrict__ h,
                                                        float* __restrict__ dw1, float* __restrict__ db1,
                                                        float* __restrict__ dw2, float* __restrict__ db2, float beta, int N,
                                                        int C, int Cr) {
  const int64_t nw = (int64_t)C * Cr, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * nw + Cr + C) return;
  float* out = i < nw ? (dw1 ? dw1 + i : nullptr)
               : i < 2 * nw ? (dw2 ? dw2 + (i - nw) : nullptr)
               : i < 2 * nw + Cr ? (db1 ? db1 + (i - 2 * nw) : nullptr) : (db2 ? db2 + (i - 2 * nw - Cr) : nullptr);
  if (!out) return;
  const float v = (float)ca_param_grad(i, da, dh, m, h, N, C, Cr);
  *out = beta == 0.f ? v : beta * *out + v;   // (beta == 0: the destination may hold anything)
}

static int ca_check_dims(int N, int H, int W, int C, const char* who) {
  SRK_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "%s: bad dims (N %d, %d x %d, C %d)", who, N, H, W, C);
  if (C > kCaMaxC) {
    set_error("%s: C = %d, at most SRK_CA_MAX_C = %d channels are supported", who, C, kCaMaxC);
    return SRK_ERR_UNSUPPORTED;
  }
  return SRK_OK;
}

static int ca_check(int N, int H, int W, int C, int Cr, const char* who) {
  if (int rc = ca_check_dims(N, H, W, C, who)) return rc;
  SRK_REQUIRE(Cr > 0, "%s: bad dims (Cr %d)", who, Cr);
  SRK_REQUIRE(Cr <= C, "%s: Cr = %d exceeds C = %d (the hidden layer reduces)", who, Cr, C);
  if (Cr > kCaMaxCr) {
    set_error("%s: Cr = %d, at most SRK_CA_MAX_CR = %d hidden channels are supported", who, Cr, kCaMaxCr);
    return SRK_ERR_UNSUPPORTED;
  }
  return SRK_OK;
}

static size_t ca_workspace(int N, int H, int W, int C) {
  return ((size_t)N * ca_splits((int64_t)H * W) * C + (size_t)2 * N * C) * sizeof(double);
}

static CaGeom ca_geom(int H, int W, int C, int Cr) {
  CaGeom q;
  q.rows = (int64_t)H * W;
  q.C = C, q.Cr = Cr;
  q.splits = ca_splits(q.rows);
  q.apply_rows = ca_apply_rows(q.splits);
  q.blocks_per_sample = (int)((q.rows + q.apply_rows - 1) / q.apply_rows);
  return q;
}

}  // namespace srk

using namespace srk;

extern "C" int srk_channel_attention_splits(int N, int H, int W, int C) {
  if (int rc = ca_check_dims(N, H, W, C, "channel_attention_splits")) return rc;
  return ca_splits((int64_t)H * W);
}

extern "C" size_t srk_channel_attention_workspace(int N, int H, int W, int C) {
  if (ca_check_dims(N, H, W, C, "channel_attention_workspace")) return 0;
  return ca_workspace(N, H, W, C);
}

extern "C" int srk_channel_attention_forward(const float* t, const float* x, const float* w1, const float* b1,
                                             const float* w2, const float* b2, int N, int H, int W, int C, int Cr, float* y,
                                             float* m, float* h, float* s, void* workspace, size_t workspace_bytes,
                                             void* stream) {
  const char* who = "channel_attention_forward";
  SRK_REQUIRE(t && w1 && b1 && w2 && b2 && y && workspace, "%s: null pointer", who);
  SRK_REQUIRE((m && h && s) || (!m && !h && !s), "%s: m, h and s are saved together or not at all", who);
  if (int rc = ca_check(N, H, W, C, Cr, who)) return rc;
  if (workspace_bytes < ca_workspace(N, H, W, C)) {
    set_error("%s: workspace of %zu bytes, srk_channel_attention_workspace says %zu", who, workspace_bytes,
              ca_workspace(N, H, W, C));
    return SRK_ERR_WORKSPACE;
  }
  const CaGeom q = ca_geom(H, W, C, Cr);
  double* partials = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g1((unsigned)N * q.splits), g2((unsigned)N * q.blocks_per_sample), blk(256);
  if (C % 4 == 0 && aligned16(t, x, y)) {
    hipLaunchKernelGGL((k_ca_colsum<4, false>), g1, blk, 0, st, t, (const float*)nullptr, partials, q.rows, C, q.splits);
    hipLaunchKernelGGL(k_ca_gate_apply<4>, g2, blk, 0, st, t, x, y, (const double*)partials, w1, b1, w2, b2, m, h, s, q);
  } else {
    hipLaunchKernelGGL((k_ca_colsum<1, false>), g1, blk, 0, st, t, (const float*)nullptr, partials, q.rows, C, q.splits);
    hipLaunchKernelGGL(k_ca_gate_apply<1>, g2, blk, 0, st, t, x, y, (const double*)partials, w1, b1, w2, b2, m, h, s, q);
  }
  return check_launch(who);
}

extern "C" int srk_channel_attention_backward(const float* g, const float* t, const float* w1, const float* w2,
                                              const float* m, const float* h, const float* s, int N, int H, int W, int C,
                                              int Cr, float* dt, float* dw1, float* db1, float* dw2, float* db2, float beta,
                                              void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "channel_attention_backward";
  SRK_REQUIRE(g && t && w1 && w2 && m && h && s && dt && workspace, "%s: null pointer", who);
  if (int rc = ca_check(N, H, W, C, Cr, who)) return rc;
  if (workspace_bytes < ca_workspace(N, H, W, C)) {
    set_error("%s: workspace of %zu bytes, srk_channel_attention_workspace says %zu", who, workspace_bytes,
              ca_workspace(N, H, W, C));
    return SRK_ERR_WORKSPACE;
  }
  const CaGeom q = ca_geom(H, W, C, Cr);
  double* partials = (double*)workspace;
  double* ws_da = partials + (size_t)N * q.splits * C;
  double* ws_dh = ws_da + (size_t)N * C;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g1((unsigned)N * q.splits), g2((unsigned)N * q.blocks_per_sample), blk(256);
  if (C % 4 == 0 && aligned16(g, t, dt)) {
    hipLaunchKernelGGL((k_ca_colsum<4, true>), g1, blk, 0, st, g, t, partials, q.rows, C, q.splits);
    hipLaunchKernelGGL(k_ca_bwd_apply<4>, g2, blk, 0, st, g, dt, (const double*)partials, w1, w2, h, s, ws_da, ws_dh, q);
  } else {
    hipLaunchKernelGGL((k_ca_colsum<1, true>), g1, blk, 0, st, g, t, partials, q.rows, C, q.splits);
    hipLaunchKernelGGL(k_ca_bwd_apply<1>, g2, blk, 0, st, g, dt, (const double*)partials, w1, w2, h, s, ws_da, ws_dh, q);
  }
  if (dw1 || db1 || dw2 || db2) {
    const int64_t outs = (int64_t)2 * C * Cr + Cr + C;
    hipLaunchKernelGGL(k_ca_param_grads, dim3(cdiv((size_t)outs, 256)), blk, 0, st, (const double*)ws_da,
                       (const double*)ws_dh, m, h, dw1, db1, dw2, db2, beta, N, C, Cr);
  }
  return check_launch(who);
}

// The same definition on host pointers, everything after the fp32 inputs in double (the device rounds m, h, s, y and dt
// to fp32), so that the definition can be pinned far below the device's rounding.  g == NULL: forward only.
extern "C" int srk_channel_attention_host(const float* t, const float* x, const float* w1, const float* b1, const float* w2,
                                          const float* b2, const float* g, int N, int H, int W, int C, int Cr, double* y,
                                          double* dt, double* dw1, double* db1, double* dw2, double* db2) {
  const char* who = "channel_attention_host";
  SRK_REQUIRE(t && w1 && b1 && w2 && b2 && y, "%s: null pointer", who);
  SRK_REQUIRE(!g || (dt && dw1 && db1 && dw2 && db2), "%s: null pointer (a backward needs dt, dw1, db1, dw2 and db2)", who);
  if (int rc = ca_check(N, H, W, C, Cr, who)) return rc;
  const int64_t rows = (int64_t)H * W;
  std::vector<double> m((size_t)N * C), h((size_t)N * Cr), s((size_t)N * C), da((size_t)N * C), dh((size_t)N * Cr), dm(C);
  for (int n = 0; n < N; ++n) {
    const float* tn = t + (size_t)n * rows * C;
    for (int c = 0; c < C; ++c) {
      double a = 0.0;
      for (int64_t r = 0; r < rows; ++r) a += (double)tn[(size_t)r * C + c];
      m[(size_t)n * C + c] = a / (double)rows;
    }
    for (int j = 0; j < Cr; ++j) h[(size_t)n * Cr + j] = ca_hidden(j, &m[(size_t)n * C], w1, b1, C);
    for (int c = 0; c < C; ++c) s[(size_t)n * C + c] = ca_gate(c, &h[(size_t)n * Cr], w2, b2, Cr);
    for (int64_t r = 0; r < rows; ++r)
      for (int c = 0; c < C; ++c) {
        const size_t i = ((size_t)n * rows + r) * C + c;
        y[i] = (double)t[i] * s[(size_t)n * C + c] + (x ? (double)x[i] : 0.0);
      }
  }
  if (!g) return SRK_OK;
  for (int n = 0; n < N; ++n) {
    const size_t base = (size_t)n * rows * C;
    for (int c = 0; c < C; ++c) {
      double a = 0.0;
      for (int64_t r = 0; r < rows; ++r) a += (double)g[base + (size_t)r * C + c] * (double)t[base + (size_t)r * C + c];
      da[(size_t)n * C + c] = ca_dgate(a, s[(size_t)n * C + c]);
    }
    for (int j = 0; j < Cr; ++j) dh[(size_t)n * Cr + j] = ca_dhidden(j, &da[(size_t)n * C], w2, &h[(size_t)n * Cr], C, Cr);
    for (int c = 0; c < C; ++c) dm[c] = ca_dmean(c, &dh[(size_t)n * Cr], w1, C, Cr) / (double)rows;
    for (int64_t r = 0; r < rows; ++r)
      for (int c = 0; c < C; ++c) dt[base + (size_t)r * C + c] = (double)g[base + (size_t)r * C + c] * s[(size_t)n * C + c] + dm[c];
  }
  const int64_t nw = (int64_t)C * Cr;
  for (int64_t i = 0; i < 2 * nw + Cr + C; ++i) {
    const double v = ca_param_grad(i, da.data(), dh.data(), m.data(), h.data(), N, C, Cr);
    (i < nw ? dw1[i] : i < 2 * nw ? dw2[i - nw] : i < 2 * nw + Cr ? db1[i - 2 * nw] : db2[i - 2 * nw - Cr]) = v;
  }
  return SRK_OK;
}
