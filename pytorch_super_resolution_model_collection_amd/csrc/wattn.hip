// Shifted-window self-attention of SwinIR, forward and backward, on an NHWC map.  Definition: include/srk.h and
// DESIGN.md 29; all index arithmetic (shift, window, relative index, mask regions) is wattn_common.h's, shared with the
// host twin at the end of this file.
//
//   forward    k_wattn_fwd<D>       one wave (= one block) per (window, head); lane i is token i.  K and V of the window are
//                                   staged in LDS and read back as broadcasts, q_i and the score row s_i[0..T) stay in
//                                   registers, so max, exp and sum need no cross-lane traffic; the roll, the partition,
//                                   the head split and their inverses are the addresses of the loads and the stores.
//   backward   k_wattn_bwd<D>       phase 1, lane i = row i: recomputes P_i. = exp(S_i. - lse_i), dS_i., dQ_i and leaves
//                                   P in LDS; phase 2, lane j = column j: dV_j, dK_j (dS recomputed from P, V_j, dO_i)
//                                   and the bias-table bins.  For a fixed i the T lanes hit T different bins, so the
//                                   block's bins are plain LDS adds in i order.
//              k_wattn_dtable       the blocks' bins added up in a fixed order, in double, one wave an element
// D = the head dimension rounded up to 8, 16 or 32 (rows are zero-padded).  A block walks windows blockIdx.x,
// blockIdx.x + gridDim.x, ... of head blockIdx.y; the grid depends on the shape alone.  No atomics.
#include <math.h>

#include <vector>

#include "srk_common.h"
#include "wattn_common.h"

namespace srk {

constexpr int kWaBlocksPerHead = 1024;   // windows beyond this many share blocks (and bins)
constexpr int kWaBinsPad = 232;         // >= (2 * 8 - 1)^2

template <int D>
__device__ __forceinline__ void wa_load_row(const float* __restrict__ p, int d, bool v2, float (&r)[D]) {
  if (v2) {
#pragma unroll
    for (int c = 0; c < D; c += 2) {
      const float2 v = c < d ? *reinterpret_cast<const float2*>(p + c) : make_float2(0.f, 0.f);
      r[c] = v.x, r[c + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) r[c] = c < d ? p[c] : 0.f;
  }
}

template <int D>
__device__ __forceinline__ void wa_store_row(float* __restrict__ p, int d, bool v2, const float (&r)[D], float mul) {
  if (v2) {
#pragma unroll
    for (int c = 0; c < D; c += 2)
      if (c < d) *reinterpret_cast<float2*>(p + c) = make_float2(r[c] * mul, r[c + 1] * mul);
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c)
      if (c < d) p[c] = r[c] * mul;
  }
}

// a lane's row of a [64][D + 4] LDS image (the pad keeps 16-byte rows off one bank group)
template <int D>
__device__ __forceinline__ void wa_lds_put(float* __restrict__ img, int lane, const float (&r)[D]) {
  f32x4* dst = reinterpret_cast<f32x4*>(img + lane * (D + 4));
#pragma unroll
  for (int c = 0; c < D; c += 4) dst[c / 4] = f32x4{r[c], r[c + 1], r[c + 2], r[c + 3]};
}
template <int D>
__device__ __forceinline__ void wa_lds_get(const float* __restrict__ img, int row, float (&r)[D]) {
  const f32x4* src = reinterpret_cast<const f32x4*>(img + row * (D + 4));
#pragma unroll
  for (int c = 0; c < D; c += 4) {
    const f32x4 v = src[c / 4];
    r[c] = v[0], r[c + 1] = v[1], r[c + 2] = v[2], r[c + 3] = v[3];
  }
}
template <int D>
__device__ __forceinline__ float wa_dot(const float (&a)[D], const float (&b)[D]) {
  // four independent chains: D dependent FMAs would wait out the FMA latency at the few waves a SIMD holds here
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int c = 0; c < D; c += 4) {
    s0 = fmaf(a[c], b[c], s0), s1 = fmaf(a[c + 1], b[c + 1], s1);
    s2 = fmaf(a[c + 2], b[c + 2], s2), s3 = fmaf(a[c + 3], b[c + 3], s3);
  }
  return (s0 + s1) + (s2 + s3);
}

// lin(t) = y_t * (2w - 1) + x_t: rel(i, j) = lin(i) - lin(j) + (w - 1) * 2w
__device__ __forceinline__ int wa_lin(int t, int window) { return (t / window) * (2 * window - 1) + t % window; }

struct WaWindow {
  int n, wy, wx;
};
__device__ __forceinline__ WaWindow wa_window(const WaGeom& g, int win) {
  const int per = g.wins_y * g.wins_x;
  WaWindow w;
  w.n = win / per;
  const int rem = win - w.n * per;
  w.wy = rem / g.wins_x, w.wx = rem - w.wy * g.wins_x;
  return w;
}

// WIN = 8: the window of both published nets at compile time -- T = 64, the relative index of column j is an immediate, and
// the unrolled loops are one basic block, so the scheduler may run the LDS reads of column j + 1 under the FMAs of column
// j.  WIN = 0: any window, one guarded block per column.
template <int D, int WIN>
__global__ __launch_bounds__(64) void k_wattn_fwd(const float* __restrict__ qkv, const float* __restrict__ table,
                                                  float* __restrict__ out, float* __restrict__ lse, WaGeom g,
                                                  int wins_total, int v2) {
  __shared__ __attribute__((aligned(16))) float sK[64 * (D + 4)];
  __shared__ __attribute__((aligned(16))) float sV[64 * (D + 4)];
  __shared__ float sT[kWaBinsPad];
  __shared__ int sL[64], sR[64];
  const int lane = threadIdx.x, h = blockIdx.y, T = WIN ? WIN * WIN : g.T, d = g.d, C = g.C;
  const int window = WIN ? WIN : g.window;
  const bool live = lane < T;
  const int t = live ? lane : 0;
  const float scale = 1.0f / sqrtf((float)d);
  for (int b = lane; b < g.bins; b += 64) sT[b] = table[(size_t)b * g.heads + h];
  sL[lane] = wa_lin(t, window);
  const int my_lin = wa_lin(t, window) + (window - 1) * 2 * window;
  for (int win = blockIdx.x; win < wins_total; win += gridDim.x) {
    const WaWindow w = wa_window(g, win);
    const int64_t pix = (int64_t)w.n * g.H * g.W + wa_token_pixel(g, w.wy, w.wx, t);
    const float* row = qkv + pix * 3 * C + h * d;
    const int my_region = wa_token_region(g, w.wy, w.wx, t);
    float q[D], r[D];
    wa_load_row<D>(row, d, v2, q);
    __syncthreads();   // the previous window's K and V have been read (first pass: nothing)
    wa_load_row<D>(row + C, d, v2, r);
    wa_lds_put<D>(sK, lane, r);
    wa_load_row<D>(row + 2 * C, d, v2, r);
    wa_lds_put<D>(sV, lane, r);
    sR[lane] = my_region;
    __syncthreads();
    float s[64];
    float m = -3.0e38f;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
      if (WIN || j < T) {
        wa_lds_get<D>(sK, j, r);
        float v = fmaf(wa_dot<D>(q, r), scale, sT[my_lin - (WIN ? wa_lin(j, WIN ? WIN : 1) : sL[j])]);
        if (g.shift != 0 && sR[j] != my_region) v += kWaMasked;
        s[j] = v;
        m = fmaxf(m, v);
      } else {
        s[j] = 0.f;
      }
    }
    float l = 0.f, o[D];
#pragma unroll
    for (int c = 0; c < D; ++c) o[c] = 0.f;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
      if (WIN || j < T) {
        const float p = __expf(s[j] - m);
        l += p;
        wa_lds_get<D>(sV, j, r);
#pragma unroll
        for (int c = 0; c < D; ++c) o[c] = fmaf(p, r[c], o[c]);
      }
    }
    if (live) {
      wa_store_row<D>(out + pix * C + h * d, d, v2, o, 1.0f / l);
      if (lse) lse[((size_t)win * g.heads + h) * 64 + lane] = m + logf(l);
    }
  }
}

template <int D>
__global__ __launch_bounds__(64) void k_wattn_bwd(const float* __restrict__ dout, const float* __restrict__ qkv,
                                                  const float* __restrict__ table, const float* __restrict__ out,
                                                  const float* __restrict__ lse, float* __restrict__ dqkv,
                                                  float* __restrict__ partials, WaGeom g, int wins_total, int v2) {
  __shared__ __attribute__((aligned(16))) float sA[64 * (D + 4)];   // K, then Q
  __shared__ __attribute__((aligned(16))) float sB[64 * (D + 4)];   // V, then dO
  __shared__ float sM[64 * 65];                                     // P[i][j] at i * 65 + j
  __shared__ float sT[kWaBinsPad], sBin[kWaBinsPad], sD[64];
  __shared__ int sL[64], sR[64];
  const int lane = threadIdx.x, h = blockIdx.y, T = g.T, d = g.d, C = g.C;
  const bool live = lane < T;
  const int t = live ? lane : 0;
  const float scale = 1.0f / sqrtf((float)d);
  for (int b = lane; b < kWaBinsPad; b += 64) {
    sT[b] = b < g.bins ? table[(size_t)b * g.heads + h] : 0.f;
    sBin[b] = 0.f;
  }
  sL[lane] = wa_lin(t, g.window);
  const int rel0 = (g.window - 1) * 2 * g.window;
  const int my_lin = wa_lin(t, g.window);
  for (int win = blockIdx.x; win < wins_total; win += gridDim.x) {
    const WaWindow w = wa_window(g, win);
    const int64_t pix = (int64_t)w.n * g.H * g.W + wa_token_pixel(g, w.wy, w.wx, t);
    const float* row = qkv + pix * 3 * C + h * d;
    float* grow = dqkv + pix * 3 * C + h * d;
    const int my_region = wa_token_region(g, w.wy, w.wx, t);
    float q[D], go[D], r[D], acc[D];
    wa_load_row<D>(row, d, v2, q);
    wa_load_row<D>(dout + pix * C + h * d, d, v2, go);
    wa_load_row<D>(out + pix * C + h * d, d, v2, r);
    const float dsum = wa_dot<D>(go, r);   // D_i = dO_i . O_i = sum_j P_ij dP_ij
    const float my_lse = lse[((size_t)win * g.heads + h) * 64 + t];
    __syncthreads();   // the previous window's phase 2 is over
    wa_load_row<D>(row + C, d, v2, r);
    wa_lds_put<D>(sA, lane, r);
    wa_load_row<D>(row + 2 * C, d, v2, r);
    wa_lds_put<D>(sB, lane, r);
    sR[lane] = my_region;
    __syncthreads();
    // phase 1: row i
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = 0.f;
#pragma unroll 2
    for (int j = 0; j < T; ++j) {
      float kj[D];
      wa_lds_get<D>(sA, j, kj);
      float s = fmaf(wa_dot<D>(q, kj), scale, sT[my_lin - sL[j] + rel0]);
      if (g.shift != 0 && sR[j] != my_region) s += kWaMasked;
      const float p = __expf(s - my_lse);
      wa_lds_get<D>(sB, j, r);
      const float ds = p * (wa_dot<D>(go, r) - dsum);
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = fmaf(ds, kj[c], acc[c]);
      sM[lane * 65 + j] = p;
    }
    if (live) wa_store_row<D>(grow, d, v2, acc, scale);   // dQ_i
    float vj[D];
    wa_lds_get<D>(sB, lane, vj);   // this lane's own V row, for phase 2
    __syncthreads();
    wa_lds_put<D>(sA, lane, q);
    wa_lds_put<D>(sB, lane, go);
    sD[lane] = dsum;
    __syncthreads();
    // phase 2: column j
    float dk[D];
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = 0.f, dk[c] = 0.f;
#pragma unroll 2
    for (int i = 0; i < T; ++i) {
      const float p = sM[i * 65 + lane];
      wa_lds_get<D>(sB, i, r);   // dO_i
      const float ds = p * (wa_dot<D>(r, vj) - sD[i]);
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = fmaf(p, r[c], acc[c]);   // dV_j
      wa_lds_get<D>(sA, i, r);   // Q_i
#pragma unroll
      for (int c = 0; c < D; ++c) dk[c] = fmaf(ds, r[c], dk[c]);
      if (live) sBin[sL[i] - my_lin + rel0] += ds;   // rel(i, j): distinct over the lanes of one step
    }
    if (live) {
      wa_store_row<D>(grow + C, d, v2, dk, scale);
      wa_store_row<D>(grow + 2 * C, d, v2, acc, 1.0f);
    }
  }
  __syncthreads();
  if (partials)
    for (int b = lane; b < g.bins; b += 64) partials[((size_t)h * gridDim.x + blockIdx.x) * g.bins + b] = sBin[b];
}

__global__ __launch_bounds__(256) void k_wattn_dtable(const float* __restrict__ partials, float* __restrict__ dtable,
                                                      float beta, int bins, int heads, int blocks) {
  // one wave an element: lane l adds blocks l, l + 64, ... in order, then the lanes are added in a fixed tree
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= bins * heads) return;
  const int b = i / heads, h = i - b * heads;
  double a = 0.0;
  for (int k = lane; k < blocks; k += 64) a += (double)partials[((size_t)h * blocks + k) * bins + b];
  a = wave_sum_d(a);
  if (lane == 0) dtable[i] = beta == 0.f ? (float)a : beta * dtable[i] + (float)a;
}

static int wa_check(int N, int H, int W, int C, int heads, int window, int shift, const char* who) {
  SRK_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && heads > 0, "%s: bad dims (N %d, %d x %d, C %d, heads %d)", who, N, H, W, C,
              heads);
  SRK_REQUIRE(window >= kWaMinWindow && window <= kWaMaxWindow, "%s: window %d, supported are %d .. %d (one lane a token)",
              who, window, kWaMinWindow, kWaMaxWindow);
  SRK_REQUIRE(shift >= 0 && shift < window, "%s: shift %d is not in [0, window = %d)", who, shift, window);
  SRK_REQUIRE(H % window == 0 && W % window == 0, "%s: %d x %d is not a multiple of the window %d", who, H, W, window);
  SRK_REQUIRE(C % heads == 0, "%s: %d heads do not divide C = %d", who, heads, C);
  SRK_REQUIRE(C / heads <= kWaMaxHeadDim, "%s: head dimension %d, at most %d is supported", who, C / heads, kWaMaxHeadDim);
  SRK_REQUIRE((int64_t)N * (H / window) * (W / window) < (int64_t)1 << 30, "%s: too many windows", who);
  return SRK_OK;
}

static int wa_blocks(int wins_total) { return wins_total < kWaBlocksPerHead ? wins_total : kWaBlocksPerHead; }

static size_t wa_workspace(int N, int H, int W, int heads, int window) {
  const int wins_total = N * (H / window) * (W / window), bins = (2 * window - 1) * (2 * window - 1);
  return (size_t)wa_blocks(wins_total) * heads * bins * sizeof(float);
}

}  // namespace srk

using namespace srk;

extern "C" size_t srk_window_attention_workspace(int N, int H, int W, int C, int heads, int window) {
  if (wa_check(N, H, W, C, heads, window, 0, "window_attention_workspace")) return 0;
  return wa_workspace(N, H, W, heads, window);
}

extern "C" int srk_window_attention_forward(const float* qkv, const float* table, int N, int H, int W, int C, int heads,
                                            int window, int shift, float* out, float* lse, void* stream) {
  const char* who = "window_attention_forward";
  SRK_REQUIRE(qkv && table && out, "%s: null pointer", who);
  if (int rc = wa_check(N, H, W, C, heads, window, shift, who)) return rc;
  const WaGeom g = wa_geom(N, H, W, C, heads, window, shift);
  const int wins_total = N * g.wins_y * g.wins_x;
  const int v2 = g.d % 2 == 0 && ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(out)) & 7) == 0;
  const dim3 grid((unsigned)wa_blocks(wins_total), (unsigned)heads), blk(64);
  hipStream_t st = (hipStream_t)stream;
  if (window == 8) {
    if (g.d <= 8)
      hipLaunchKernelGGL((k_wattn_fwd<8, 8>), grid, blk, 0, st, qkv, table, out, lse, g, wins_total, v2);
    else if (g.d <= 16)
      hipLaunchKernelGGL((k_wattn_fwd<16, 8>), grid, blk, 0, st, qkv, table, out, lse, g, wins_total, v2);
    else
      hipLaunchKernelGGL((k_wattn_fwd<32, 8>), grid, blk, 0, st, qkv, table, out, lse, g, wins_total, v2);
  } else if (g.d <= 8) {
    hipLaunchKernelGGL((k_wattn_fwd<8, 0>), grid, blk, 0, st, qkv, table, out, lse, g, wins_total, v2);
  } else if (g.d <= 16) {
    hipLaunchKernelGGL((k_wattn_fwd<16, 0>), grid, blk, 0, st, qkv, table, out, lse, g, wins_total, v2);
  } else {
    hipLaunchKernelGGL((k_wattn_fwd<32, 0>), grid, blk, 0, st, qkv, table, out, lse, g, wins_total, v2);
  }
  return check_launch(who);
}

extern "C" int srk_window_attention_backward(const float* dout, const float* qkv, const float* table, const float* out,
                                             const float* lse, int N, int H, int W, int C, int heads, int window,
                                             int shift, float* dqkv, float* dtable, float beta, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  const char* who = "window_attention_backward";
  SRK_REQUIRE(dout && qkv && table && out && lse && dqkv, "%s: null pointer", who);
  SRK_REQUIRE(!dtable || workspace, "%s: null pointer (dtable needs the workspace)", who);
  if (int rc = wa_check(N, H, W, C, heads, window, shift, who)) return rc;
  if (dtable && workspace_bytes < wa_workspace(N, H, W, heads, window)) {
    set_error("%s: workspace of %zu bytes, srk_window_attention_workspace says %zu", who, workspace_bytes,
              wa_workspace(N, H, W, heads, window));
    return SRK_ERR_WORKSPACE;
  }
  const WaGeom g = wa_geom(N, H, W, C, heads, window, shift);
  const int wins_total = N * g.wins_y * g.wins_x, blocks = wa_blocks(wins_total);
  const int v2 = g.d % 2 == 0 && ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(out) |
                                   reinterpret_cast<uintptr_t>(dout) | reinterpret_cast<uintptr_t>(dqkv)) & 7) == 0;
  const dim3 grid((unsigned)blocks, (unsigned)heads), blk(64);
  hipStream_t st = (hipStream_t)stream;
  float* partials = dtable ? (float*)workspace : nullptr;
  if (g.d <= 8)
    hipLaunchKernelGGL(k_wattn_bwd<8>, grid, blk, 0, st, dout, qkv, table, out, lse, dqkv, partials, g, wins_total, v2);
  else if (g.d <= 16)
    hipLaunchKernelGGL(k_wattn_bwd<16>, grid, blk, 0, st, dout, qkv, table, out, lse, dqkv, partials, g, wins_total, v2);
  else
    hipLaunchKernelGGL(k_wattn_bwd<32>, grid, blk, 0, st, dout, qkv, table, out, lse, dqkv, partials, g, wins_total, v2);
  if (dtable)
    hipLaunchKernelGGL(k_wattn_dtable, dim3(cdiv((size_t)g.bins * heads, 4)), dim3(256), 0, st, (const float*)partials,
                       dtable, beta, g.bins, heads, blocks);
  return check_launch(who);
}

// The definition on host pointers, in double, window by window from wattn_common.h's loop.  dout == NULL: forward only.
extern "C" int srk_window_attention_host(const float* qkv, const float* table, const float* dout, int N, int H, int W,
                                         int C, int heads, int window, int shift, double* out, double* dqkv,
                                         double* dtable) {
  const char* who = "window_attention_host";
  SRK_REQUIRE(qkv && table && out, "%s: null pointer", who);
  SRK_REQUIRE(!dout || (dqkv && dtable), "%s: null pointer (a backward needs dqkv and dtable)", who);
  if (int rc = wa_check(N, H, W, C, heads, window, shift, who)) return rc;
  const WaGeom g = wa_geom(N, H, W, C, heads, window, shift);
  if (dout)
    for (int i = 0; i < g.bins * heads; ++i) dtable[i] = 0.0;
  for (int n = 0; n < N; ++n)
    for (int wy = 0; wy < g.wins_y; ++wy)
      for (int wx = 0; wx < g.wins_x; ++wx)
        for (int h = 0; h < heads; ++h) wa_window_reference<double>(g, qkv, table, n, wy, wx, h, out, dout, dqkv, dtable);
  return SRK_OK;
}

// The header's index functions for the CPU suite: region id of the token at shifted (r, c), relative index of (ti, tj),
// and the pixel a window's token is read from and written to.
extern "C" int srk_window_attention_region(int H, int W, int window, int shift, int r, int c) {
  if (wa_check(1, H, W, 1, 1, window, shift, "window_attention_region") || r < 0 || r >= H || c < 0 || c >= W) return -1;
  const WaGeom g = wa_geom(1, H, W, 1, 1, window, shift);
  return shift == 0 ? 0 : wa_region(g, r, c);
}
extern "C" int srk_window_attention_rel_index(int window, int ti, int tj) {
  if (window < kWaMinWindow || window > kWaMaxWindow || ti < 0 || tj < 0 || ti >= window * window || tj >= window * window)
    return -1;
  return wa_rel_index(ti, tj, window);
}
extern "C" int64_t srk_window_attention_token_pixel(int H, int W, int window, int shift, int wy, int wx, int t) {
  if (wa_check(1, H, W, 1, 1, window, shift, "window_attention_token_pixel") || wy < 0 || wy >= H / window || wx < 0 ||
      wx >= W / window || t < 0 || t >= window * window)
    return -1;
  return wa_token_pixel(wa_geom(1, H, W, 1, 1, window, shift), wy, wx, t);
}
