// The SSIM training loss, 1 - mean(SSIM) of an unclamped prediction against its target (float domain, L = 1), with its
// gradient from the same launch.  Definition: include/srk.h and DESIGN.md 20; window, constants and formula are those of
// the evaluation kernel (ssim_common.h).
//
// k_ssim_loss: a block owns kLossTH x kLossTW PIXELS of dpred (of up to kLossMaxPlanes channels of one image, one plane
// after the other).  A pixel gathers from the positions whose window holds it, positions from the pixels of their window,
// so per plane the block stages the tile plus a 20-pixel halo of both tensors (zero outside the plane), then
//   horizontal pass   five fp64 row sums at the tile plus 10 columns                      -> LDS
//   vertical pass     five fp64 moments at the tile plus 10 positions each way, formula:
//                     S, summed where the block owns the position (the tile that holds the position's first pixel),
//                     and the three coefficient maps dS/dmx, dS/dexx, dS/dexy, zero where there is no position -> LDS
//   adjoint passes    the window again, horizontally then vertically, as GATHERS over the coefficient maps,
//                     dpred = -grad_scale / M * (G^T pm + 2 x G^T pxx + y G^T pxy)
// Nothing image-sized reaches memory but dpred.  Per-block sums of S go to the workspace in double, k_ssim_loss_final
// adds them in a fixed order: no atomics, two calls give the same bits.  All arithmetic is double: on flat planes the
// three gradient terms are ~1/C2 times their sum.
#include <vector>

#include "ssim_common.h"

namespace srk {

// pixels of dpred per block and plane (16 x 16 beat 8 x 32, 32 x 16 and 16 x 32 by 1.15 - 1.28x: DESIGN 20)
constexpr int kLossTH = 16, kLossTW = 16;
constexpr int kLossSH = kLossTH + 2 * kSsimHalo, kLossSW = kLossTW + 2 * kSsimHalo;   // staged pixels: 36 x 36
constexpr int kLossPH = kLossTH + kSsimHalo, kLossPW = kLossTW + kSsimHalo;           // positions: 26 x 26
constexpr int kLossMaxPlanes = 4;      // channels one block takes, one after the other
constexpr int kLossPartials = 8192;    // blocks of a launch at most
constexpr int kLossHB = 4, kLossHChunks = (kLossPW + kLossHB - 1) / kLossHB;   // horizontal pass: columns per thread
constexpr int kLossChunks = 256 / kLossPW;                                  // vertical pass: row chunks per column
constexpr int kLossRows = (kLossPH + kLossChunks - 1) / kLossChunks;        // ... and position rows per thread
static_assert(kLossChunks >= 1 && kLossChunks * kLossRows >= kLossPH, "the vertical pass covers every position row");
static_assert(5 * kLossSH * kLossPW >= 3 * kLossPH * kLossTW, "the adjoint's row sums fit where the moments' were");

struct SsimLossJob {
  const float* pred;   // NHWC dense
  const float* gt;
  float* dpred;        // NHWC dense, or NULL
  Strides4 gs;
  int C, H, W;
  int cgroups;         // groups of up to kLossMaxPlanes channels
  int tiles_y, tiles_x;
  int64_t ntiles;      // N * cgroups * tiles_y * tiles_x
  double scale;        // -grad_scale / M
};

constexpr size_t kLossLds = (size_t)2 * kLossSH * kLossSW * sizeof(float) + (size_t)5 * kLossSH * kLossPW * sizeof(double) +
                            (size_t)3 * kLossPH * kLossPW * sizeof(double) +
                            (size_t)kLossMaxPlanes * kLossTH * kLossTW * sizeof(float);
static_assert((2 * kLossSH * kLossSW * sizeof(float)) % 8 == 0, "the doubles behind the staged floats are aligned");

__global__ __launch_bounds__(256) void k_ssim_loss(SsimLossJob job, double* __restrict__ partials) {
  extern __shared__ __align__(16) unsigned char loss_lds[];
  __shared__ double sm[4];
  float* sx = reinterpret_cast<float*>(loss_lds);                 // [SH][SW]
  float* sy = sx + kLossSH * kLossSW;                             // [SH][SW]
  double* hs = reinterpret_cast<double*>(sy + kLossSH * kLossSW); // [5][SH][PW]; later the adjoint's row sums [3][PH][TW]
  double* cf = hs + 5 * kLossSH * kLossPW;                        // [3][PH][PW]
  float* ob = reinterpret_cast<float*>(cf + 3 * kLossPH * kLossPW);   // [planes][TH][TW]: dpred of the tile, all planes
  const int MH = job.H - kSsimHalo, MW = job.W - kSsimHalo;
  const int tid = threadIdx.x;
  const int vcol = tid % kLossPW, vchunk = tid / kLossPW;         // vertical pass: a column and a run of rows
  double ssum = 0.0;

  for (int64_t t = blockIdx.x; t < job.ntiles; t += gridDim.x) {
    int64_t u = t;
    const int tx = (int)(u % job.tiles_x);
    u /= job.tiles_x;
    const int ty = (int)(u % job.tiles_y);
    u /= job.tiles_y;
    const int cg = (int)(u % job.cgroups);
    const int64_t n = u / job.cgroups;
    const int c0 = cg * kLossMaxPlanes;
    const int planes = job.C - c0 < kLossMaxPlanes ? job.C - c0 : kLossMaxPlanes;
    const int y0 = ty * kLossTH, x0 = tx * kLossTW;          // the tile's first pixel; staging starts 10 before it
    const float* pbase = job.pred + n * (int64_t)job.H * job.W * job.C;
    const float* gbase = job.gt + n * job.gs.n;

    for (int p = 0; p < planes; ++p) {
      const int ch = c0 + p;
      for (int i = tid; i < kLossSH * kLossSW; i += 256) {
        const int r = i / kLossSW, c = i - r * kLossSW;
        const int gy = y0 - kSsimHalo + r, gx = x0 - kSsimHalo + c;
        float a = 0.f, b = 0.f;
        if (gy >= 0 && gy < job.H && gx >= 0 && gx < job.W) {
          a = pbase[((int64_t)gy * job.W + gx) * job.C + ch];
          b = gbase[(int64_t)ch * job.gs.c + (int64_t)gy * job.gs.h + (int64_t)gx * job.gs.w];
        }
        sx[i] = a, sy[i] = b;
      }
      __syncthreads();

      // horizontal: five row sums per staged row and position column; a thread takes kLossHB neighbouring columns, so
      // every pixel is read, widened and squared once per thread, not once per tap
      for (int i = tid; i < kLossSH * kLossHChunks; i += 256) {
        const int r = i / kLossHChunks, j0 = (i - r * kLossHChunks) * kLossHB;
        double m[kLossHB][5];
#pragma unroll
        for (int jj = 0; jj < kLossHB; ++jj)
#pragma unroll
          for (int q = 0; q < 5; ++q) m[jj][q] = 0.0;
#pragma unroll
        for (int t = 0; t < kLossHB + kSsimHalo; ++t) {
          // (columns past the staged ones feed only position columns >= kLossPW, which are not stored)
          const int col = j0 + t < kLossSW ? j0 + t : kLossSW - 1;
          const double a = sx[r * kLossSW + col], b = sy[r * kLossSW + col];
          const double aa = a * a, bb = b * b, ab = a * b;
#pragma unroll
          for (int jj = 0; jj < kLossHB; ++jj) {
            const int k = t - jj;
            if (k >= 0 && k < kSsimTaps) {
              const double g = kSsimWinDev.g[k];
              m[jj][0] = fma(g, a, m[jj][0]), m[jj][1] = fma(g, b, m[jj][1]);
              m[jj][2] = fma(g, aa, m[jj][2]), m[jj][3] = fma(g, bb, m[jj][3]), m[jj][4] = fma(g, ab, m[jj][4]);
            }
          }
        }
#pragma unroll
        for (int jj = 0; jj < kLossHB; ++jj)
          if (j0 + jj < kLossPW) {
#pragma unroll
            for (int q = 0; q < 5; ++q) hs[(q * kLossSH + r) * kLossPW + j0 + jj] = m[jj][q];
          }
      }
      __syncthreads();

      if (vchunk < kLossChunks) {   // vertical: each row sum feeds the thread's kLossRows positions
        double acc[kLossRows][5];
#pragma unroll
        for (int j = 0; j < kLossRows; ++j)
#pragma unroll
          for (int q = 0; q < 5; ++q) acc[j][q] = 0.0;
        const int r0 = vchunk * kLossRows;
#pragma unroll
        for (int rr = 0; rr < kLossRows + kSsimHalo; ++rr) {
          // (rows past the staged ones feed only position rows >= kLossPH, which are dropped below)
          const int row = r0 + rr < kLossSH ? r0 + rr : kLossSH - 1;
          double h[5];
#pragma unroll
          for (int q = 0; q < 5; ++q) h[q] = hs[(q * kLossSH + row) * kLossPW + vcol];
#pragma unroll
          for (int j = 0; j < kLossRows; ++j) {
            const int k = rr - j;
            if (k >= 0 && k < kSsimTaps) {
#pragma unroll
              for (int q = 0; q < 5; ++q) acc[j][q] = fma(kSsimWinDev.g[k], h[q], acc[j][q]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < kLossRows; ++j) {
          const int pi = r0 + j;
          if (pi < kLossPH) {
            const int gi = y0 - kSsimHalo + pi, gj = x0 - kSsimHalo + vcol;   // the position (its window's first pixel)
            double pm = 0.0, pxx = 0.0, pxy = 0.0;
            if (gi >= 0 && gi < MH && gj >= 0 && gj < MW) {
              const double s = ssim_loss_terms(acc[j][0], acc[j][1], acc[j][2], acc[j][3], acc[j][4], pm, pxx, pxy);
              if (pi >= kSsimHalo && vcol >= kSsimHalo) ssum += s;   // the position's first pixel lies in this tile
            }
            cf[(0 * kLossPH + pi) * kLossPW + vcol] = pm;
            cf[(1 * kLossPH + pi) * kLossPW + vcol] = pxx;
            cf[(2 * kLossPH + pi) * kLossPW + vcol] = pxy;
          }
        }
      }
      __syncthreads();

      if (job.dpred) {
        // adjoint, horizontal: pixel column c of the tile (staged column c + 10) is tap k of position column c + 10 - k
        double* ts = hs;   // [3][PH][TW]
        for (int i = tid; i < 3 * kLossPH * kLossTW; i += 256) {
          const int c = i % kLossTW, mr = i / kLossTW;   // mr = map * PH + position row
          double a = 0.0;
#pragma unroll
          for (int k = 0; k < kSsimTaps; ++k) a = fma(kSsimWinDev.g[k], cf[mr * kLossPW + c + kSsimHalo - k], a);
          ts[i] = a;
        }
        __syncthreads();
        // adjoint, vertical: pixel row r of the tile is tap k of position row r + 10 - k
        for (int i = tid; i < kLossTH * kLossTW; i += 256) {
          const int r = i / kLossTW, c = i - r * kLossTW;
          double u[3] = {0.0, 0.0, 0.0};
#pragma unroll
          for (int k = 0; k < kSsimTaps; ++k)
#pragma unroll
            for (int m = 0; m < 3; ++m)
              u[m] = fma(kSsimWinDev.g[k], ts[(m * kLossPH + r + kSsimHalo - k) * kLossTW + c], u[m]);
          const int si = (r + kSsimHalo) * kLossSW + c + kSsimHalo;
          const double x = sx[si], y = sy[si];
          ob[p * kLossTH * kLossTW + i] = (float)(job.scale * (u[0] + 2.0 * x * u[1] + y * u[2]));
        }
      }
      __syncthreads();   // sx / sy / hs / cf are written again
    }

    if (job.dpred) {   // the tile's pixels, channel fastest as dpred holds them
      float* dbase = job.dpred + n * (int64_t)job.H * job.W * job.C;
      for (int i = tid; i < planes * kLossTH * kLossTW; i += 256) {
        const int p = i % planes, pix = i / planes;
        const int r = pix / kLossTW, c = pix - r * kLossTW;
        if (y0 + r < job.H && x0 + c < job.W)
          dbase[((int64_t)(y0 + r) * job.W + x0 + c) * job.C + c0 + p] = ob[p * kLossTH * kLossTW + pix];
      }
      __syncthreads();   // ob is written again
    }
  }
  const double s_tot = block_sum_256_d(ssum, sm);
  if (tid == 0) partials[blockIdx.x] = s_tot;
}

__global__ __launch_bounds__(256) void k_ssim_loss_final(const double* __restrict__ partials, int nparts, double positions,
                                                         float* __restrict__ loss) {
  __shared__ double sm[4];
  const double s_tot = sum_partials_256_d(partials, nparts, sm);
  if (threadIdx.x == 0) *loss = (float)(1.0 - s_tot / positions);
}

// the argument rules the device call and the host twin share
static int ssim_loss_check(const void* pred, const void* gt, const void* loss, int N, int C, int H, int W,
                           const char* who) {
  SRK_REQUIRE(pred && gt && loss, "%s: null pointer", who);
  SRK_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "%s: bad dims (N %d, C %d, %d x %d)", who, N, C, H, W);
  SRK_REQUIRE(H >= kSsimTaps && W >= kSsimTaps, "%s: a plane of %d x %d is smaller than the %d x %d window", who, H, W,
              kSsimTaps, kSsimTaps);
  return SRK_OK;
}

static inline Strides4 ssim_loss_strides(const int64_t* s, int C, int H, int W) {
  if (s) return {s[0], s[1], s[2], s[3]};
  return {(int64_t)H * W * C, 1, (int64_t)W * C, C};   // NULL: NHWC-dense, as srk_loss_forward_backward
}

}  // namespace srk

using namespace srk;

extern "C" size_t srk_ssim_loss_workspace_bytes(void) { return (size_t)kLossPartials * sizeof(double); }

extern "C" int srk_ssim_loss_forward_backward(const float* pred, const float* target, const int64_t* target_strides, int N,
                                              int C, int H, int W, float grad_scale, float* loss, float* dpred,
                                              void* workspace, void* stream) {
  if (int rc = ssim_loss_check(pred, target, loss, N, C, H, W, "ssim_loss")) return rc;
  SRK_REQUIRE(workspace, "ssim_loss: null workspace");
  SsimLossJob job;
  job.pred = pred, job.gt = target, job.dpred = dpred;
  job.gs = ssim_loss_strides(target_strides, C, H, W);
  job.C = C, job.H = H, job.W = W;
  job.cgroups = (int)cdiv(C, kLossMaxPlanes);
  job.tiles_y = (int)cdiv(H, kLossTH);
  job.tiles_x = (int)cdiv(W, kLossTW);
  job.ntiles = (int64_t)N * job.cgroups * job.tiles_y * job.tiles_x;
  const double positions = (double)N * C * (H - kSsimHalo) * (double)(W - kSsimHalo);
  job.scale = -(double)grad_scale / positions;
  const int nb = (int)(job.ntiles < kLossPartials ? job.ntiles : kLossPartials);
  hipStream_t s = (hipStream_t)stream;
  launch_lds<&k_ssim_loss>(dim3(nb), dim3(256), kLossLds, s, job, (double*)workspace);
  hipLaunchKernelGGL(k_ssim_loss_final, dim3(1), dim3(256), 0, s, (const double*)workspace, nb, positions, loss);
  return check_launch("ssim_loss_forward_backward");
}

// The same definition in plain C++ double on host pointers, one plane at a time; dpred (NHWC-dense, may be NULL) in
// double, so that the definition can be pinned far below the fp32 of the device's output.
extern "C" int srk_ssim_loss_host(const float* pred, const float* target, const int64_t* target_strides, int N, int C, int H,
                                  int W, double grad_scale, double* loss, double* dpred) {
  if (int rc = ssim_loss_check(pred, target, loss, N, C, H, W, "ssim_loss_host")) return rc;
  const Strides4 gs = ssim_loss_strides(target_strides, C, H, W);
  const int mh = H - kSsimHalo, mw = W - kSsimHalo;
  const double positions = (double)N * C * mh * (double)mw;
  const double scale = -grad_scale / positions;
  const double* g = kSsimWinHost.g;
  std::vector<double> x((size_t)H * W), y((size_t)H * W), hs((size_t)5 * H * mw), cf((size_t)3 * mh * mw),
      ts((size_t)3 * mh * W);
  double ssum = 0.0;
  for (int n = 0; n < N; ++n)
    for (int ch = 0; ch < C; ++ch) {
      for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
          x[(size_t)r * W + c] = pred[(((int64_t)n * H + r) * W + c) * C + ch];
          y[(size_t)r * W + c] = target[n * gs.n + ch * gs.c + (int64_t)r * gs.h + (int64_t)c * gs.w];
        }
      for (int r = 0; r < H; ++r)
        for (int c = 0; c < mw; ++c) {
          double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
          for (int k = 0; k < kSsimTaps; ++k) {
            const double a = x[(size_t)r * W + c + k], b = y[(size_t)r * W + c + k];
            m[0] = fma(g[k], a, m[0]), m[1] = fma(g[k], b, m[1]);
            m[2] = fma(g[k], a * a, m[2]), m[3] = fma(g[k], b * b, m[3]), m[4] = fma(g[k], a * b, m[4]);
          }
          for (int q = 0; q < 5; ++q) hs[((size_t)q * H + r) * mw + c] = m[q];
        }
      for (int r = 0; r < mh; ++r)
        for (int c = 0; c < mw; ++c) {
          double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
          for (int k = 0; k < kSsimTaps; ++k)
            for (int q = 0; q < 5; ++q) m[q] = fma(g[k], hs[((size_t)q * H + r + k) * mw + c], m[q]);
          double pm, pxx, pxy;
          ssum += ssim_loss_terms(m[0], m[1], m[2], m[3], m[4], pm, pxx, pxy);
          cf[((size_t)0 * mh + r) * mw + c] = pm;
          cf[((size_t)1 * mh + r) * mw + c] = pxx;
          cf[((size_t)2 * mh + r) * mw + c] = pxy;
        }
      if (!dpred) continue;
      for (int mr = 0; mr < 3 * mh; ++mr)   // adjoint, horizontal: pixel column c is tap k of position column c - k
        for (int c = 0; c < W; ++c) {
          double a = 0.0;
          for (int k = 0; k < kSsimTaps; ++k)
            if (c - k >= 0 && c - k < mw) a = fma(g[k], cf[(size_t)mr * mw + c - k], a);
          ts[(size_t)mr * W + c] = a;
        }
      for (int r = 0; r < H; ++r)           // adjoint, vertical: pixel row r is tap k of position row r - k
        for (int c = 0; c < W; ++c) {
          double u[3] = {0.0, 0.0, 0.0};
          for (int k = 0; k < kSsimTaps; ++k)
            if (r - k >= 0 && r - k < mh)
              for (int m = 0; m < 3; ++m) u[m] = fma(g[k], ts[((size_t)m * mh + r - k) * W + c], u[m]);
          const double xv = x[(size_t)r * W + c], yv = y[(size_t)r * W + c];
          dpred[(((int64_t)n * H + r) * W + c) * C + ch] = scale * (u[0] + 2.0 * xv * u[1] + yv * u[2]);
        }
    }
  *loss = 1.0 - ssum / positions;
  return SRK_OK;
}
