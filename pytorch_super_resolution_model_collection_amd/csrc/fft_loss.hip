// The frequency-domain training loss: mean |Re F| + |Im F| (halved) of the 2-D DFT of pred - target, per plane, with its
// gradient.  Definition: include/srk.h and DESIGN.md 26.  A dense fp64 DFT (planes of at most 256 x 256): four small GEMMs
// per plane against the H x H and W x W DFT matrices, whose entries are DATA (srk_dft_table_host, uploaded by the
// caller) addressed by (u * y) mod n -- no cos / sin on the device.  d is real, so only columns v = 0 .. W/2 of the
// spectrum are computed (column v stands for W - v too: F[-u,-v] = conj F[u,v], and so for the sign image and for its
// adjoint column transform).
//
//   k_fft_diff      d = pred - target in double, planar and TRANSPOSED: d[plane][x][y]                   (workspace)
//   k_fft_rows      row pass             T[plane][y][v] = sum_x d[y,x] w_W^(v x)          lanes: rows y of all planes
//   k_fft_cols      column pass          F[u][v] = sum_y T[y][v] w_H^(u y); |Re| + |Im| summed per block, the signs
//                                        G[u][plane, v] stored as four bytes a bin         lanes: columns v of all planes
//   k_fft_cols_adj  adjoint column pass  S[plane][v][y] = sum_u G[u][v] conj(w_H)^(u y)   lanes: columns v of all planes
//   k_fft_grad      adjoint row pass     dpred[y,x] = g * Re sum_v m_v S[y][v] conj(w_W)^(v x)   lanes: rows y
//   k_fft_final     the block sums of k_fft_cols in index order -> loss
//
// The one idea of all four GEMM kernels: the 64 lanes of a wave run along the dimension that is NOT transformed, and a
// lane keeps 4 outputs along the one that is, for each of its two entries (lane l owns l and l + 64 of a wave's 128).  The twiddle of (output, step) is then the same for every lane: its index
// is wave-uniform, it is walked in scalar registers (fft_tw_next) and the table entry arrives through the scalar cache,
// so the vector side of an inner step is two coalesced loads and 16 or 32 fp64 FMAs.  A work item is one wave's 128 x 4
// outputs, so a batch of 48 planes still fills the device; the loads of the next four steps are issued before the
// arithmetic of the current four (fft_stream).  No LDS but k_fft_diff's tile and the block sum's, no atomics anywhere: two calls give the same
// bits.  Everything is double up to the two fp32 stores (dpred, loss).
#include <vector>

#include "fft_loss_common.h"

namespace srk {

constexpr int kFftMaxDim = SRK_FFT_LOSS_MAX_DIM;
constexpr int kFftOut = 4;             // outputs a lane keeps along the transformed dimension, for each of ...
constexpr int kFftSets = 2;            // ... its rows (columns): lane l of a wave owns entries l and l + 64 of 128
constexpr int kFftSpan = 64 * kFftSets;
constexpr int kFftAhead = 4;           // steps whose operands are loaded ahead of the arithmetic
constexpr int kFftPartials = 1024;     // blocks of a GEMM launch at most (4 waves a SIMD on 256 CUs); beyond, a wave takes several items

constexpr int kFftTile = 16;           // k_fft_diff transposes tiles of 16 x 16 pixels ...
constexpr int kFftTileC = 4;           // ... of up to 4 channels at a time

struct FftDiffJob {
  const float* pred;   // NHWC dense
  const float* gt;
  Strides4 gs;
  int C, H, W;
  int tiles_y, tiles_x, cgroups;
  int64_t ntiles;      // N * tiles_y * tiles_x * cgroups
};

// d[plane][x][y] = (double)pred - (double)target.  A block takes 16 x 16 pixels of up to 4 channels of one image: it
// reads them along pred's memory (channel fastest, then x) and writes them along d's (y fastest), through LDS.
__global__ __launch_bounds__(256) void k_fft_diff(FftDiffJob job, double* __restrict__ d) {
  __shared__ double tile[kFftTileC][kFftTile][kFftTile + 1];
  for (int64_t t = blockIdx.x; t < job.ntiles; t += gridDim.x) {
    int64_t u = t;
    const int c0 = (int)(u % job.cgroups) * kFftTileC;
    u /= job.cgroups;
    const int x0 = (int)(u % job.tiles_x) * kFftTile;
    u /= job.tiles_x;
    const int y0 = (int)(u % job.tiles_y) * kFftTile;
    const int64_t n = u / job.tiles_y;
    const int nc = job.C - c0 < kFftTileC ? job.C - c0 : kFftTileC;
    for (int i = threadIdx.x; i < kFftTile * kFftTile * nc; i += 256) {
      const int cc = i % nc, xx = (i / nc) % kFftTile, yy = i / (nc * kFftTile);
      const int y = y0 + yy, x = x0 + xx, c = c0 + cc;
      if (y < job.H && x < job.W) {
        const double a = job.pred[((n * job.H + y) * job.W + x) * job.C + c];
        const double b = job.gt[n * job.gs.n + (int64_t)c * job.gs.c + (int64_t)y * job.gs.h + (int64_t)x * job.gs.w];
        tile[cc][xx][yy] = a - b;
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kFftTile * kFftTile * nc; i += 256) {
      const int yy = i % kFftTile, xx = (i / kFftTile) % kFftTile, cc = i / (kFftTile * kFftTile);
      const int y = y0 + yy, x = x0 + xx, c = c0 + cc;
      if (y < job.H && x < job.W) d[((n * job.C + c) * job.W + x) * job.H + y] = tile[cc][xx][yy];
    }
    __syncthreads();   // the tile is written again
  }
}

// The operands of one step: one value for each of the lane's kFftSets rows (columns).
template <typename V>
struct FftOperands {
  V s[kFftSets];
};

// step(load(i)) for i = 0 .. n-1 in order, n >= 1, with the loads kFftAhead steps ahead of their use.  Loads past the
// end repeat the last element (in bounds) and are not used.
template <typename V, typename Load, typename Step>
__device__ __forceinline__ void fft_stream(int n, Load load, Step step) {
  FftOperands<V> cur[kFftAhead], nxt[kFftAhead];
#pragma unroll
  for (int j = 0; j < kFftAhead; ++j) cur[j] = load(j < n ? j : n - 1);
  for (int i0 = 0; i0 < n; i0 += kFftAhead) {
#pragma unroll
    for (int j = 0; j < kFftAhead; ++j) {
      const int i = i0 + kFftAhead + j;
      nxt[j] = load(i < n ? i : n - 1);
    }
#pragma unroll
    for (int j = 0; j < kFftAhead; ++j)
      if (i0 + j < n) step(cur[j]);
#pragma unroll
    for (int j = 0; j < kFftAhead; ++j) cur[j] = nxt[j];
  }
}

// The wave-uniform walk through a twiddle table of n entries, in BYTES (one scalar add, compare, select, subtract a step
// and the offset goes into the scalar load as it is): entry (step * i) mod n at step i.
struct FftWalk {
  unsigned off, step, bytes;
  __device__ __forceinline__ void start(int stride, int n) {
    off = 0u, step = (unsigned)stride * (unsigned)sizeof(FftTw), bytes = (unsigned)n * (unsigned)sizeof(FftTw);
  }
  __device__ __forceinline__ FftTw next(const FftTw* __restrict__ tw) {
    const FftTw w = *reinterpret_cast<const FftTw*>(reinterpret_cast<const char*>(tw) + off);
    off = (unsigned)fft_tw_next((int)off, (int)step, (int)bytes);
    return w;
  }
};

// One wave's share of the 128 entries (rows or columns) of item group `grp`: entry, whether it exists, and the entry to
// read instead if it does not (the last one: idle lanes compute on it and store nothing).
struct FftLaneSet {
  int64_t e[kFftSets];
  bool live[kFftSets];
  __device__ __forceinline__ FftLaneSet(int64_t grp, int lane, int64_t total) {
#pragma unroll
    for (int s = 0; s < kFftSets; ++s) {
      const int64_t i = grp * kFftSpan + s * 64 + lane;
      live[s] = i < total;
      e[s] = live[s] ? i : total - 1;
    }
  }
};

// Row pass.  A wave takes 128 rows (plane, y) and kFftOut columns v of the half spectrum.
__global__ __launch_bounds__(256) void k_fft_rows(const double* __restrict__ d, const FftTw* __restrict__ twW,
                                                  double2* __restrict__ T, int64_t rows, int H, int W, int64_t nitems,
                                                  int vgroups) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nhv = fft_half_cols(W);
  for (int64_t it = (int64_t)blockIdx.x * 4 + wave; it < nitems; it += (int64_t)gridDim.x * 4) {
    const int v0 = (int)(it % vgroups) * kFftOut;
    const FftLaneSet ls(it / vgroups, lane, rows);
    const double* dp[kFftSets];
    double2* tp[kFftSets];
#pragma unroll
    for (int s = 0; s < kFftSets; ++s) {
      const int64_t p = ls.e[s] / H;
      const int y = (int)(ls.e[s] - p * H);
      dp[s] = d + p * (int64_t)W * H + y;
      tp[s] = T + ls.e[s] * nhv;                     // T[plane][y][v]: (plane * H + y) is the row index itself
    }
    FftWalk walk[kFftOut];
    double re[kFftSets][kFftOut], im[kFftSets][kFftOut];
#pragma unroll
    for (int k = 0; k < kFftOut; ++k) {
      walk[k].start(v0 + k < nhv ? v0 + k : nhv - 1, W);   // (columns past the half repeat its last one, not stored)
#pragma unroll
      for (int s = 0; s < kFftSets; ++s) re[s][k] = 0.0, im[s][k] = 0.0;
    }
    fft_stream<double>(W,
                       [&](int x) {
                         FftOperands<double> o;
#pragma unroll
                         for (int s = 0; s < kFftSets; ++s) o.s[s] = dp[s][(int64_t)x * H];
                         return o;
                       },
                       [&](const FftOperands<double>& o) {
#pragma unroll
                         for (int k = 0; k < kFftOut; ++k) {
                           const FftTw w = walk[k].next(twW);
#pragma unroll
                           for (int s = 0; s < kFftSets; ++s) fft_fwd_real(o.s[s], w, re[s][k], im[s][k]);
                         }
                       });
#pragma unroll
    for (int s = 0; s < kFftSets; ++s)
      if (ls.live[s]) {
#pragma unroll
        for (int k = 0; k < kFftOut; ++k)
          if (v0 + k < nhv) tp[s][v0 + k] = make_double2(re[s][k], im[s][k]);
      }
  }
}

// Column pass, the bins' terms and signs.  A wave takes 128 columns (plane, v) and kFftOut rows u of the spectrum.
__global__ __launch_bounds__(256) void k_fft_cols(const double2* __restrict__ T, const FftTw* __restrict__ twH,
                                                  ushort2* __restrict__ G, double* __restrict__ partials, int64_t cols, int H,
                                                  int W, int64_t nitems, int ugroups) {
  __shared__ double sm[4];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nhv = fft_half_cols(W);
  double lsum = 0.0;
  for (int64_t it = (int64_t)blockIdx.x * 4 + wave; it < nitems; it += (int64_t)gridDim.x * 4) {
    const int u0 = (int)(it % ugroups) * kFftOut;
    const FftLaneSet ls(it / ugroups, lane, cols);
    const double2* tp[kFftSets];
    double wt[kFftSets];
#pragma unroll
    for (int s = 0; s < kFftSets; ++s) {
      const int64_t p = ls.e[s] / nhv;
      const int v = (int)(ls.e[s] - p * nhv);
      wt[s] = fft_col_is_edge(v, W) ? 1.0 : 2.0;     // an inner column stands for its mirror too
      tp[s] = T + p * (int64_t)H * nhv + v;
    }
    FftWalk walk[kFftOut];
    double re[kFftSets][kFftOut], im[kFftSets][kFftOut];
#pragma unroll
    for (int k = 0; k < kFftOut; ++k) {
      walk[k].start(u0 + k < H ? u0 + k : H - 1, H);
#pragma unroll
      for (int s = 0; s < kFftSets; ++s) re[s][k] = 0.0, im[s][k] = 0.0;
    }
    fft_stream<double2>(H,
                        [&](int y) {
                          FftOperands<double2> o;
#pragma unroll
                          for (int s = 0; s < kFftSets; ++s) o.s[s] = tp[s][(int64_t)y * nhv];
                          return o;
                        },
                        [&](const FftOperands<double2>& o) {
#pragma unroll
                          for (int k = 0; k < kFftOut; ++k) {
                            const FftTw w = walk[k].next(twH);
#pragma unroll
                            for (int s = 0; s < kFftSets; ++s) fft_fwd_cplx(o.s[s].x, o.s[s].y, w, re[s][k], im[s][k]);
                          }
                        });
#pragma unroll
    for (int s = 0; s < kFftSets; ++s)
      if (ls.live[s]) {
#pragma unroll
        for (int k = 0; k < kFftOut; ++k)
          if (u0 + k < H) {
            if (G) G[(int64_t)(u0 + k) * cols + ls.e[s]] = make_ushort2(fft_sign_code(re[s][k]), fft_sign_code(im[s][k]));
            lsum += wt[s] * fft_bin_term(re[s][k], im[s][k]);
          }
      }
  }
  store_block_sum_256_d(lsum, sm, partials + blockIdx.x);
}

// Adjoint column pass.  A wave takes 128 columns (plane, v) and kFftOut rows y.
__global__ __launch_bounds__(256) void k_fft_cols_adj(const ushort2* __restrict__ G, const FftTw* __restrict__ twH,
                                                      double2* __restrict__ S, int64_t cols, int H, int64_t nitems,
                                                      int ygroups) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t it = (int64_t)blockIdx.x * 4 + wave; it < nitems; it += (int64_t)gridDim.x * 4) {
    const int y0 = (int)(it % ygroups) * kFftOut;
    const FftLaneSet ls(it / ygroups, lane, cols);
    FftWalk walk[kFftOut];
    double re[kFftSets][kFftOut], im[kFftSets][kFftOut];
#pragma unroll
    for (int k = 0; k < kFftOut; ++k) {
      walk[k].start(y0 + k < H ? y0 + k : H - 1, H);
#pragma unroll
      for (int s = 0; s < kFftSets; ++s) re[s][k] = 0.0, im[s][k] = 0.0;
    }
    fft_stream<ushort2>(H,
                      [&](int u) {
                        FftOperands<ushort2> o;
#pragma unroll
                        for (int s = 0; s < kFftSets; ++s) o.s[s] = G[(int64_t)u * cols + ls.e[s]];
                        return o;
                      },
                      [&](const FftOperands<ushort2>& o) {
                        double gr[kFftSets], gi[kFftSets];
#pragma unroll
                        for (int s = 0; s < kFftSets; ++s) gr[s] = fft_sign_decode(o.s[s].x), gi[s] = fft_sign_decode(o.s[s].y);
#pragma unroll
                        for (int k = 0; k < kFftOut; ++k) {
                          const FftTw w = walk[k].next(twH);
#pragma unroll
                          for (int s = 0; s < kFftSets; ++s) fft_adj_cplx(gr[s], gi[s], w, re[s][k], im[s][k]);
                        }
                      });
#pragma unroll
    for (int s = 0; s < kFftSets; ++s)
      if (ls.live[s]) {
        double2* sp = S + ls.e[s] * (int64_t)H;      // S[plane][v][y]: (plane * nhv + v) is the column index itself
#pragma unroll
        for (int k = 0; k < kFftOut; ++k)
          if (y0 + k < H) sp[y0 + k] = make_double2(re[s][k], im[s][k]);
      }
  }
}

// Adjoint row pass.  A wave takes 128 rows (plane, y) and kFftOut pixels x; the two edge columns of the half spectrum
// count once, the others twice (they stand for their mirrors).
__global__ __launch_bounds__(256) void k_fft_grad(const double2* __restrict__ S, const FftTw* __restrict__ twW,
                                                  float* __restrict__ dpred, int64_t rows, int C, int H, int W,
                                                  int64_t nitems, int xgroups, double gscale) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nhv = fft_half_cols(W);
  const int vmid_end = (W % 2 == 0) ? nhv - 1 : nhv;   // an even W ends on the Nyquist column, an edge
  for (int64_t it = (int64_t)blockIdx.x * 4 + wave; it < nitems; it += (int64_t)gridDim.x * 4) {
    const int x0 = (int)(it % xgroups) * kFftOut;
    const FftLaneSet ls(it / xgroups, lane, rows);
    const double2* sp[kFftSets];
    float* op[kFftSets];
#pragma unroll
    for (int s = 0; s < kFftSets; ++s) {
      const int64_t p = ls.e[s] / H;
      const int y = (int)(ls.e[s] - p * H);
      const int64_t n = p / C;
      sp[s] = S + p * (int64_t)nhv * H + y;
      op[s] = dpred + ((n * H + y) * (int64_t)W) * C + (p - n * C);
    }
    FftWalk walk[kFftOut];
    double edge[kFftSets][kFftOut], mid[kFftSets][kFftOut];
#pragma unroll
    for (int k = 0; k < kFftOut; ++k) walk[k].start(x0 + k < W ? x0 + k : W - 1, W);
#pragma unroll
    for (int s = 0; s < kFftSets; ++s) {
      const double2 z = sp[s][0];
#pragma unroll
      for (int k = 0; k < kFftOut; ++k) {
        edge[s][k] = 0.0, mid[s][k] = 0.0;
        fft_adj_real(z.x, z.y, twW[0], edge[s][k]);
      }
    }
#pragma unroll
    for (int k = 0; k < kFftOut; ++k) walk[k].next(twW);    // past v = 0
    if (vmid_end > 1)
      fft_stream<double2>(vmid_end - 1,
                          [&](int i) {
                            FftOperands<double2> o;
#pragma unroll
                            for (int s = 0; s < kFftSets; ++s) o.s[s] = sp[s][(int64_t)(i + 1) * H];
                            return o;
                          },
                          [&](const FftOperands<double2>& o) {
#pragma unroll
                            for (int k = 0; k < kFftOut; ++k) {
                              const FftTw w = walk[k].next(twW);
#pragma unroll
                              for (int s = 0; s < kFftSets; ++s) fft_adj_real(o.s[s].x, o.s[s].y, w, mid[s][k]);
                            }
                          });
    if (vmid_end < nhv && vmid_end > 0) {
#pragma unroll
      for (int k = 0; k < kFftOut; ++k) {
        const FftTw w = walk[k].next(twW);
#pragma unroll
        for (int s = 0; s < kFftSets; ++s) {
          const double2 z = sp[s][(int64_t)vmid_end * H];
          fft_adj_real(z.x, z.y, w, edge[s][k]);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < kFftSets; ++s)
      if (ls.live[s]) {
#pragma unroll
        for (int k = 0; k < kFftOut; ++k)
          if (x0 + k < W) op[s][(int64_t)(x0 + k) * C] = (float)(gscale * fma(2.0, mid[s][k], edge[s][k]));
      }
  }
}

__global__ __launch_bounds__(256) void k_fft_final(const double* __restrict__ partials, int nparts, double lscale,
                                                   float* __restrict__ loss) {
  __shared__ double sm[4];
  const double tot = sum_partials_256_d(partials, nparts, sm);
  if (threadIdx.x == 0) *loss = (float)(lscale * tot);
}

// the argument rules the device call and the host twin share
static int fft_loss_check(const void* pred, const void* gt, const void* loss, int N, int C, int H, int W, double scale,
                          const char* who) {
  SRK_REQUIRE(pred && gt && loss, "%s: null pointer", who);
  SRK_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "%s: bad dims (N %d, C %d, %d x %d)", who, N, C, H, W);
  SRK_REQUIRE(scale > 0.0 && scale < INFINITY, "%s: scale %g is not a positive finite number", who, scale);
  if (H > kFftMaxDim || W > kFftMaxDim) {
    set_error("%s: a plane of %d x %d, at most SRK_FFT_LOSS_MAX_DIM = %d on a side is supported (the DFT is dense)", who, H,
              W, kFftMaxDim);
    return SRK_ERR_UNSUPPORTED;
  }
  return SRK_OK;
}

static inline Strides4 fft_loss_strides(const int64_t* s, int C, int H, int W) {
  if (s) return {s[0], s[1], s[2], s[3]};
  return {(int64_t)H * W * C, 1, (int64_t)W * C, C};   // NULL: NHWC-dense, as srk_loss_forward_backward
}

struct FftLayout {
  int64_t planes, cols, col_items;
  size_t t_bytes, s_bytes;   // T [planes][H][nhv] and S [planes][nhv][H] (d [planes][W][H] lives in S's place first)
  size_t g_bytes;            // G [H][planes * nhv], four bytes a bin (fft_sign_code)
  int nparts;                // blocks of k_fft_cols
};
static inline FftLayout fft_layout(int N, int C, int H, int W) {
  FftLayout l;
  l.planes = (int64_t)N * C;
  l.cols = l.planes * fft_half_cols(W);
  l.col_items = ((l.cols + kFftSpan - 1) / kFftSpan) * ((H + kFftOut - 1) / kFftOut);
  l.t_bytes = (size_t)l.cols * H * sizeof(double2);
  l.s_bytes = l.t_bytes;     // >= planes * W * H doubles: 2 * (W / 2 + 1) > W
  l.g_bytes = (((size_t)l.cols * H * sizeof(ushort2)) + 15) / 16 * 16;
  l.nparts = (int)grid_for((size_t)l.col_items, 4, kFftPartials);
  return l;
}

}  // namespace srk

using namespace srk;

extern "C" int srk_dft_table_host(int n, double* cos_sin) {
  SRK_REQUIRE(n > 0 && cos_sin, "dft_table_host: n = %d, table %p", n, (void*)cos_sin);
  const long double tau = 6.283185307179586476925286766559L;
  for (int k = 0; k < n; ++k) {
    double c, s;
    if ((4 * (int64_t)k) % n == 0) {        // a multiple of a quarter turn: exact
      const int q = (int)(4 * (int64_t)k / n);
      c = q == 0 ? 1.0 : (q == 2 ? -1.0 : 0.0);
      s = q == 1 ? 1.0 : (q == 3 ? -1.0 : 0.0);
    } else if (2 * (int64_t)k < n) {
      const long double a = tau * (long double)k / (long double)n;
      c = (double)cosl(a), s = (double)sinl(a);
    } else {                                // the conjugate of entry n - k, to the bit
      c = cos_sin[2 * (n - k)], s = -cos_sin[2 * (n - k) + 1];
    }
    cos_sin[2 * k] = c, cos_sin[2 * k + 1] = s;
  }
  return SRK_OK;
}

extern "C" size_t srk_fft_loss_workspace_bytes(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || H > kFftMaxDim || W > kFftMaxDim) return 0;
  const FftLayout l = fft_layout(N, C, H, W);
  return l.t_bytes + l.s_bytes + l.g_bytes + (size_t)kFftPartials * sizeof(double);
}

extern "C" int srk_fft_loss_forward_backward(const float* pred, const float* target, const int64_t* target_strides, int N,
                                             int C, int H, int W, const double* tables, double scale, float grad_scale,
                                             float* loss, float* dpred, void* workspace, void* stream) {
  if (int rc = fft_loss_check(pred, target, loss, N, C, H, W, scale, "fft_loss")) return rc;
  SRK_REQUIRE(tables, "fft_loss: null twiddle tables");
  SRK_REQUIRE(workspace, "fft_loss: null workspace");
  const FftLayout l = fft_layout(N, C, H, W);
  const int nhv = fft_half_cols(W);
  double2* T = (double2*)workspace;
  double2* S = (double2*)((char*)workspace + l.t_bytes);
  double* d = (double*)S;
  ushort2* G = (ushort2*)((char*)workspace + l.t_bytes + l.s_bytes);
  double* partials = (double*)((char*)workspace + l.t_bytes + l.s_bytes + l.g_bytes);
  const FftTw* twH = (const FftTw*)tables;
  const FftTw* twW = twH + H;
  const int64_t rows = l.planes * H;
  const int64_t rgroups = (rows + kFftSpan - 1) / kFftSpan;
  const double M = (double)N * C * H * (double)W;
  hipStream_t s = (hipStream_t)stream;

  FftDiffJob dj;
  dj.pred = pred, dj.gt = target, dj.gs = fft_loss_strides(target_strides, C, H, W);
  dj.C = C, dj.H = H, dj.W = W;
  dj.tiles_y = (int)cdiv(H, kFftTile), dj.tiles_x = (int)cdiv(W, kFftTile), dj.cgroups = (int)cdiv(C, kFftTileC);
  dj.ntiles = (int64_t)N * dj.tiles_y * dj.tiles_x * dj.cgroups;
  hipLaunchKernelGGL(k_fft_diff, dim3(grid_for((size_t)dj.ntiles, 1, 1 << 20)), dim3(256), 0, s, dj, d);
  const int vgroups = (nhv + kFftOut - 1) / kFftOut;
  const int64_t row_items = rgroups * vgroups;
  hipLaunchKernelGGL(k_fft_rows, dim3(grid_for((size_t)row_items, 4, kFftPartials)), dim3(256), 0, s, (const double*)d, twW, T, rows,
                     H, W, row_items, vgroups);
  const int ugroups = (H + kFftOut - 1) / kFftOut;
  hipLaunchKernelGGL(k_fft_cols, dim3(l.nparts), dim3(256), 0, s, (const double2*)T, twH, dpred ? G : (ushort2*)nullptr, partials,
                     l.cols, H, W, l.col_items, ugroups);
  if (dpred) {
    hipLaunchKernelGGL(k_fft_cols_adj, dim3(grid_for((size_t)l.col_items, 4, kFftPartials)), dim3(256), 0, s, (const ushort2*)G, twH, S,
                       l.cols, H, l.col_items, ugroups);
    const int xgroups = (W + kFftOut - 1) / kFftOut;
    const int64_t grad_items = rgroups * xgroups;
    hipLaunchKernelGGL(k_fft_grad, dim3(grid_for((size_t)grad_items, 4, kFftPartials)), dim3(256), 0, s, (const double2*)S, twW,
                       dpred, rows, C, H, W, grad_items, xgroups, scale * (double)grad_scale / (2.0 * M));
  }
  hipLaunchKernelGGL(k_fft_final, dim3(1), dim3(256), 0, s, (const double*)partials, l.nparts, scale / (2.0 * M), loss);
  return check_launch("fft_loss_forward_backward");
}

// The same definition in plain C++ double on host pointers: the FULL spectrum, one plane at a time, bins added in the
// order (n, c, u, v); dpred (NHWC-dense, may be NULL) in double.  Tables from srk_dft_table_host, arithmetic from
// fft_loss_common.h: what differs from the kernels is the order of the sums and that no mirror is used.
extern "C" int srk_fft_loss_host(const float* pred, const float* target, const int64_t* target_strides, int N, int C, int H,
                                 int W, double scale, double grad_scale, double* loss, double* dpred) {
  if (int rc = fft_loss_check(pred, target, loss, N, C, H, W, scale, "fft_loss_host")) return rc;
  const Strides4 gs = fft_loss_strides(target_strides, C, H, W);
  std::vector<double> tabH((size_t)2 * H), tabW((size_t)2 * W);
  srk_dft_table_host(H, tabH.data());
  srk_dft_table_host(W, tabW.data());
  const FftTw* twH = reinterpret_cast<const FftTw*>(tabH.data());
  const FftTw* twW = reinterpret_cast<const FftTw*>(tabW.data());
  const double M = (double)N * C * H * (double)W;
  const double gscale = scale * grad_scale / (2.0 * M);
  const size_t hw = (size_t)H * W;
  std::vector<double> d(hw), tr(hw), ti(hw), gr(hw), gi(hw), sr(hw), si(hw);
  double sum = 0.0;
  for (int n = 0; n < N; ++n)
    for (int ch = 0; ch < C; ++ch) {
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
          d[(size_t)y * W + x] = (double)pred[(((int64_t)n * H + y) * W + x) * C + ch] -
                                 (double)target[n * gs.n + ch * gs.c + (int64_t)y * gs.h + (int64_t)x * gs.w];
      for (int y = 0; y < H; ++y)           // row pass
        for (int v = 0; v < W; ++v) {
          double re = 0.0, im = 0.0;
          for (int x = 0, idx = 0; x < W; ++x, idx = fft_tw_next(idx, v, W)) fft_fwd_real(d[(size_t)y * W + x], twW[idx], re, im);
          tr[(size_t)y * W + v] = re, ti[(size_t)y * W + v] = im;
        }
      for (int u = 0; u < H; ++u)           // column pass, the bin's term and its sign
        for (int v = 0; v < W; ++v) {
          double re = 0.0, im = 0.0;
          for (int y = 0, idx = 0; y < H; ++y, idx = fft_tw_next(idx, u, H))
            fft_fwd_cplx(tr[(size_t)y * W + v], ti[(size_t)y * W + v], twH[idx], re, im);
          sum += fft_bin_term(re, im);
          gr[(size_t)u * W + v] = fft_sign(re), gi[(size_t)u * W + v] = fft_sign(im);
        }
      if (!dpred) continue;
      for (int y = 0; y < H; ++y)           // adjoint column pass
        for (int v = 0; v < W; ++v) {
          double re = 0.0, im = 0.0;
          for (int u = 0, idx = 0; u < H; ++u, idx = fft_tw_next(idx, y, H))
            fft_adj_cplx(gr[(size_t)u * W + v], gi[(size_t)u * W + v], twH[idx], re, im);
          sr[(size_t)y * W + v] = re, si[(size_t)y * W + v] = im;
        }
      for (int y = 0; y < H; ++y)           // adjoint row pass
        for (int x = 0; x < W; ++x) {
          double re = 0.0;
          for (int v = 0, idx = 0; v < W; ++v, idx = fft_tw_next(idx, x, W))
            fft_adj_real(sr[(size_t)y * W + v], si[(size_t)y * W + v], twW[idx], re);
          dpred[(((int64_t)n * H + y) * W + x) * C + ch] = gscale * re;
        }
    }
  *loss = scale / (2.0 * M) * sum;
  return SRK_OK;
}
