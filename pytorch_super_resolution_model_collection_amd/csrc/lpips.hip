// LPIPS (Zhang et al. 2018, the VGG variant): the distance of one tapped layer, forward and backward.  Definition:
// include/srk.h and DESIGN.md 27; the arithmetic of a pixel is lpips_common.h's, shared with the host twin.
//
//   forward    k_lpips<V, R, false>   per block the fp64 sum of d over its pixels of one sample          -> [N][blocks]
//              k_lpips_row            one block a sample adds the partials up in a fixed order, / HW      -> table[row][n]
//   finish     k_lpips_finish         the L rows added in order: values[n], their mean, the upstream vector seed / N
//   backward   k_lpips<V, R, true>    the norms again from f0 and f1, df0 written once per element
//
// f0, f1 and df0 are [N][H][W][C], channels innermost.  L lanes share a pixel (a power of two, lpips_plan): lane j keeps
// the channel groups j, j + L, ... (V floats each) of both maps in registers, the two sums of squares go across the L
// lanes by xor shuffles, and q = f0 / a - f1 / b is formed from the held values: every feature element is read once.  More
// than kLpipsMaxHeld groups a lane (C > 2048 on the 16-byte path, C > 512 on the scalar one) do not fit: R = 0 reads the
// pixel a second time.  The lanes of a pixel always own the same channels, so they keep w in registers as well.
// V = 4 floats an access where C % 4 == 0 and the pointers sit on 16-byte boundaries, else V = 1.  No atomics: a fixed
// grid, a fixed order inside the lane, the shuffle tree and the block, so two calls give the same bits.
#include <math.h>

#include "lpips_common.h"
#include "srk_common.h"

namespace srk {

// sum over the L lanes that share a pixel (the group starts at a multiple of L); every lane gets the total
__device__ __forceinline__ double lpips_group_sum(double v, int L) {
  for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct LpipsGeom {
  int64_t rows;   // H * W
  int C, G, L, blocks;
};

template <int V, int R, bool BWD>
__global__ __launch_bounds__(256) void k_lpips(const float* f0, const float* f1, const float* __restrict__ w,
                                               double* __restrict__ partials, const double* __restrict__ gout,
                                               float* __restrict__ df0, LpipsGeom q) {
  typedef typename Vec<V>::T T;
  constexpr int HELD = R > 0 ? R : 1;
  __shared__ double sm[4];
  const int G = q.G, L = q.L, tid = threadIdx.x;
  const int j = tid & (L - 1), slot = tid / L, pixels_per_pass = 256 / L;
  const int n = blockIdx.x / q.blocks, b = blockIdx.x - n * q.blocks;
  const int64_t per = (q.rows + q.blocks - 1) / q.blocks;
  const int64_t r0 = (int64_t)b * per < q.rows ? (int64_t)b * per : q.rows;
  const int64_t r1 = r0 + per < q.rows ? r0 + per : q.rows;
  T zero;
#pragma unroll
  for (int e = 0; e < V; ++e) Vec<V>::set(zero, e, 0.f);
  T wv[HELD];
  if (R > 0) {
#pragma unroll
    for (int k = 0; k < HELD; ++k) wv[k] = j + k * L < G ? Vec<V>::load(w, (size_t)(j + k * L)) : zero;
  }
  const double up = BWD ? gout[n] / (double)q.rows : 0.0;
  double acc = 0.0;
  for (int64_t p0 = r0; p0 < r1; p0 += pixels_per_pass) {   // (the same trip count for every thread of the block)
    const int64_t p = p0 + slot;
    const bool live = p < r1;
    const size_t base = ((size_t)n * q.rows + (live ? p : r0)) * G;   // in units of V floats
    T h0[HELD], h1[HELD];
    double ss0 = 0.0, ss1 = 0.0;
    if (R > 0) {
#pragma unroll
      for (int k = 0; k < HELD; ++k) {
        const bool ok = live && j + k * L < G;
        h0[k] = ok ? Vec<V>::load(f0, base + j + k * L) : zero;
        h1[k] = ok ? Vec<V>::load(f1, base + j + k * L) : zero;
      }
#pragma unroll
      for (int k = 0; k < HELD; ++k)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          ss0 = lpips_ss(Vec<V>::at(h0[k], e), ss0);
          ss1 = lpips_ss(Vec<V>::at(h1[k], e), ss1);
        }
    } else if (live) {
      for (int i = j; i < G; i += L) {
        const T a = Vec<V>::load(f0, base + i), c = Vec<V>::load(f1, base + i);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          ss0 = lpips_ss(Vec<V>::at(a, e), ss0);
          ss1 = lpips_ss(Vec<V>::at(c, e), ss1);
        }
      }
    }
    ss0 = lpips_group_sum(ss0, L);
    ss1 = lpips_group_sum(ss1, L);
    const double ia = lpips_inv_norm(ss0), ib = lpips_inv_norm(ss1);
    double d = 0.0, S = 0.0;
    if (R > 0) {
#pragma unroll
      for (int k = 0; k < HELD; ++k)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float x0 = Vec<V>::at(h0[k], e), wk = Vec<V>::at(wv[k], e);
          const double qq = lpips_q(x0, Vec<V>::at(h1[k], e), ia, ib);
          if (BWD) S = lpips_pull_term(wk, qq, x0, S);
          else d = lpips_term(wk, qq, d);
        }
    } else if (live) {
      for (int i = j; i < G; i += L) {
        const T a = Vec<V>::load(f0, base + i), c = Vec<V>::load(f1, base + i), ww = Vec<V>::load(w, (size_t)i);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const double qq = lpips_q(Vec<V>::at(a, e), Vec<V>::at(c, e), ia, ib);
          if (BWD) S = lpips_pull_term(Vec<V>::at(ww, e), qq, Vec<V>::at(a, e), S);
          else d = lpips_term(Vec<V>::at(ww, e), qq, d);
        }
      }
    }
    if (!BWD) {
      d = lpips_group_sum(d, L);
      if (j == 0 && live) acc += d;
      continue;
    }
    S = lpips_group_sum(S, L);
    const double pull = lpips_pull(ss0, ia, S);
    if (R > 0) {
#pragma unroll
      for (int k = 0; k < HELD; ++k) {
        if (!(live && j + k * L < G)) continue;
        T o;
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float x0 = Vec<V>::at(h0[k], e), wk = Vec<V>::at(wv[k], e);
          Vec<V>::set(o, e, (float)lpips_grad(x0, wk, lpips_q(x0, Vec<V>::at(h1[k], e), ia, ib), ia, pull, up));
        }
        Vec<V>::store(df0, base + j + k * L, o);
      }
    } else if (live) {
      for (int i = j; i < G; i += L) {
        const T a = Vec<V>::load(f0, base + i), c = Vec<V>::load(f1, base + i), ww = Vec<V>::load(w, (size_t)i);
        T o;
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float x0 = Vec<V>::at(a, e);
          Vec<V>::set(o, e, (float)lpips_grad(x0, Vec<V>::at(ww, e), lpips_q(x0, Vec<V>::at(c, e), ia, ib), ia, pull, up));
        }
        Vec<V>::store(df0, base + i, o);
      }
    }
  }
  if (!BWD) store_block_sum_256_d(acc, sm, partials + blockIdx.x);
}

// table[row][n] = the sample's partials added in a fixed order, over HW
__global__ __launch_bounds__(256) void k_lpips_row(const double* __restrict__ partials, double* __restrict__ out, int blocks,
                                                   int64_t rows) {
  __shared__ double sm[4];
  const double tot = sum_partials_256_d(partials + (size_t)blockIdx.x * blocks, blocks, sm);
  if (threadIdx.x == 0) out[blockIdx.x] = tot / (double)rows;
}

// values[n] = the L rows added in order; mean = their mean; gvec[n] = seed / N, what the layer backwards take
__global__ __launch_bounds__(256) void k_lpips_finish(const double* __restrict__ table, int L, int N, double seed,
                                                      float* __restrict__ values, float* __restrict__ mean,
                                                      double* __restrict__ gvec) {
  __shared__ double sm[4];
  double acc = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) {
    double v = 0.0;
    for (int l = 0; l < L; ++l) v += table[(size_t)l * N + n];
    if (values) values[n] = (float)v;
    if (gvec) gvec[n] = seed / (double)N;
    acc += v;
  }
  const double tot = block_sum_256_d(acc, sm);
  if (threadIdx.x == 0 && mean) *mean = (float)(tot / (double)N);
}

static int lpips_check_dims(int N, int H, int W, int C, const char* who) {
  SRK_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "%s: bad dims (N %d, %d x %d, C %d)", who, N, H, W, C);
  SRK_REQUIRE((int64_t)N * kLpipsMaxBlocks < INT32_MAX, "%s: N = %d samples exceed the grid", who, N);
  return SRK_OK;
}

static LpipsGeom lpips_geom(int H, int W, int C, const LpipsPlan& p) {
  LpipsGeom q;
  q.rows = (int64_t)H * W;
  q.C = C, q.G = p.G, q.L = p.L, q.blocks = p.blocks;
  return q;
}

// the larger of the two paths' partial tables: which one runs depends on the pointers
static size_t lpips_workspace(int H, int W, int C, int N) {
  const int a = lpips_plan((int64_t)H * W, C, false).blocks;
  const int b = C % 4 == 0 ? lpips_plan((int64_t)H * W, C, true).blocks : 0;
  return (size_t)N * (a > b ? a : b) * sizeof(double);
}

template <bool BWD>
static void lpips_launch(const LpipsPlan& p, const LpipsGeom& q, int N, hipStream_t st, const float* f0, const float* f1,
                         const float* w, double* partials, const double* gout, float* df0) {
  const dim3 grid((unsigned)N * q.blocks), blk(256);
#define SRK_LPIPS_CASE(VV, RR)                                                                           \
  if (p.V == VV && p.R == RR) {                                                                          \
    hipLaunchKernelGGL((k_lpips<VV, RR, BWD>), grid, blk, 0, st, f0, f1, w, partials, gout, df0, q);     \
    return;                                                                                              \
  }
  SRK_LPIPS_CASE(4, 1) SRK_LPIPS_CASE(4, 2) SRK_LPIPS_CASE(4, 4) SRK_LPIPS_CASE(4, 8) SRK_LPIPS_CASE(4, 0)
  SRK_LPIPS_CASE(1, 1) SRK_LPIPS_CASE(1, 2) SRK_LPIPS_CASE(1, 4) SRK_LPIPS_CASE(1, 8) SRK_LPIPS_CASE(1, 0)
#undef SRK_LPIPS_CASE
}

}  // namespace srk

using namespace srk;

extern "C" size_t srk_lpips_layer_workspace(int N, int H, int W, int C) {
  if (lpips_check_dims(N, H, W, C, "lpips_layer_workspace")) return 0;
  return lpips_workspace(H, W, C, N);
}

extern "C" int srk_lpips_layer_blocks(int N, int H, int W, int C, int vec) {
  if (int rc = lpips_check_dims(N, H, W, C, "lpips_layer_blocks")) return rc;
  SRK_REQUIRE(!vec || C % 4 == 0, "lpips_layer_blocks: the 16-byte path needs C %% 4 == 0 (C %d)", C);
  return lpips_plan((int64_t)H * W, C, vec != 0).blocks;
}

extern "C" int srk_lpips_layer_forward(const float* f0, const float* f1, const float* w, int N, int H, int W, int C, int row,
                                       int L, double* table, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "lpips_layer_forward";
  SRK_REQUIRE(f0 && f1 && w && table && workspace, "%s: null pointer", who);
  if (int rc = lpips_check_dims(N, H, W, C, who)) return rc;
  SRK_REQUIRE(L > 0 && row >= 0 && row < L, "%s: row %d of a table of %d rows", who, row, L);
  if (workspace_bytes < lpips_workspace(H, W, C, N)) {
    set_error("%s: workspace of %zu bytes, srk_lpips_layer_workspace says %zu", who, workspace_bytes,
              lpips_workspace(H, W, C, N));
    return SRK_ERR_WORKSPACE;
  }
  const LpipsPlan p = lpips_plan((int64_t)H * W, C, C % 4 == 0 && aligned16(f0, f1, w));
  const LpipsGeom q = lpips_geom(H, W, C, p);
  hipStream_t st = (hipStream_t)stream;
  double* partials = (double*)workspace;
  lpips_launch<false>(p, q, N, st, f0, f1, w, partials, nullptr, nullptr);
  hipLaunchKernelGGL(k_lpips_row, dim3((unsigned)N), dim3(256), 0, st, (const double*)partials, table + (size_t)row * N,
                     q.blocks, q.rows);
  return check_launch(who);
}

extern "C" int srk_lpips_finish(const double* table, int L, int N, double seed, float* values, float* mean, double* gvec,
                                void* stream) {
  const char* who = "lpips_finish";
  SRK_REQUIRE(table && (values || mean), "%s: null pointer", who);
  SRK_REQUIRE(L > 0 && N > 0, "%s: bad dims (L %d, N %d)", who, L, N);
  hipLaunchKernelGGL(k_lpips_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, table, L, N, seed, values, mean, gvec);
  return check_launch(who);
}

extern "C" int srk_lpips_layer_backward(const float* f0, const float* f1, const float* w, const double* gout, int N, int H,
                                        int W, int C, float* df0, void* stream) {
  const char* who = "lpips_layer_backward";
  SRK_REQUIRE(f0 && f1 && w && gout && df0, "%s: null pointer", who);
  if (int rc = lpips_check_dims(N, H, W, C, who)) return rc;
  const LpipsPlan p = lpips_plan((int64_t)H * W, C, C % 4 == 0 && aligned16(f0, f1, w, df0));
  const LpipsGeom q = lpips_geom(H, W, C, p);
  lpips_launch<true>(p, q, N, (hipStream_t)stream, f0, f1, w, nullptr, gout, df0);
  return check_launch(who);
}

// The same definition on host pointers, in double throughout (the device rounds df0 to fp32): value[n] = the mean of d over
// the sample's pixels; with gout (per-sample upstream gradients) df0 = gout[n] / HW * dd/df0.  gout == NULL: forward only.
extern "C" int srk_lpips_layer_host(const float* f0, const float* f1, const float* w, const double* gout, int N, int H, int W,
                                    int C, double* value, double* df0) {
  const char* who = "lpips_layer_host";
  SRK_REQUIRE(f0 && f1 && w && value, "%s: null pointer", who);
  SRK_REQUIRE(!gout == !df0, "%s: gout and df0 are given together or not at all", who);
  if (int rc = lpips_check_dims(N, H, W, C, who)) return rc;
  const int64_t rows = (int64_t)H * W;
  for (int n = 0; n < N; ++n) {
    double tot = 0.0;
    for (int64_t r = 0; r < rows; ++r) {
      const size_t base = ((size_t)n * rows + r) * C;
      double ss0 = 0.0, ss1 = 0.0;
      for (int c = 0; c < C; ++c) ss0 = lpips_ss(f0[base + c], ss0), ss1 = lpips_ss(f1[base + c], ss1);
      const double ia = lpips_inv_norm(ss0), ib = lpips_inv_norm(ss1);
      double d = 0.0, S = 0.0;
      for (int c = 0; c < C; ++c) {
        const double qq = lpips_q(f0[base + c], f1[base + c], ia, ib);
        d = lpips_term(w[c], qq, d);
        S = lpips_pull_term(w[c], qq, f0[base + c], S);
      }
      tot += d;
      if (!gout) continue;
      const double pull = lpips_pull(ss0, ia, S), up = gout[n] / (double)rows;
      for (int c = 0; c < C; ++c)
        df0[base + c] = lpips_grad(f0[base + c], w[c], lpips_q(f0[base + c], f1[base + c], ia, ib), ia, pull, up);
    }
    value[n] = tot / (double)rows;
  }
  return SRK_OK;
}
