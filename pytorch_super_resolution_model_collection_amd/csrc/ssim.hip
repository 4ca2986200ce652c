// SSIM (Wang, Bovik, Sheikh, Simoncelli 2004; 11 x 11 Gaussian window, sigma 1.5, valid positions) of a prediction against
// its target on the device, with MSE / PSNR of the same pixels from the same pass, in one of three domains: the fp32
// tensors as utils.PSNR compares them, the 8-bit picture that save_img writes, or that picture's Pillow luma.  Neither the
// cropped, nor the quantised, nor the luma picture ever exists in memory.  DESIGN.md 18.
//
// k_ssim_partial: a block owns kSsimTH x kSsimTW map positions of one image (all its channels when C <= 4), stages those
// plus the 10-pixel halo of both tensors through their element strides into LDS (domain applied on the way), then per
// plane: horizontal pass -> five fp64 row sums in LDS, vertical pass -> five fp64 moments in registers, formula, sum.
// Per-block sums go to the workspace in double; k_ssim_final adds them in a fixed order.  No atomics: two calls on the
// same inputs give the same bits.
#include <vector>

#include "ssim_common.h"

namespace srk {

constexpr int kSsimTH = 8, kSsimTW = 64;   // map positions per block (8 x 64 beat 16 x 64 by 1.14 - 1.22x: DESIGN 18)
constexpr int kSsimSH = kSsimTH + kSsimHalo, kSsimSW = kSsimTW + kSsimHalo;  // staged pixels per plane: 18 x 74
constexpr int kSsimPlane = kSsimSH * kSsimSW;
constexpr int kSsimMaxPlanes = 4;     // channels one block takes together
constexpr int kSsimPartials = 8192;   // blocks of a launch at most: {sum of ssim, sum of squared differences} each
constexpr int kSsimRowsPerThread = kSsimTH / 4;  // vertical pass: the 4 waves share the tile's rows
static_assert(kSsimTW == kWave && kSsimTH % 4 == 0, "a wave spans the tile's columns, four waves its rows");

struct SsimStrides {
  int64_t n, c, h, w;
};

struct SsimJob {
  const float* pred;
  const float* gt;
  SsimStrides ps, gs;
  int C;        // channels a block reads per pixel
  int planes;   // planes a block evaluates: C, or 1 for the luma of three channels
  int cgroups;  // blocks along the channels of one tile (C > kSsimMaxPlanes: one channel each)
  int H, W;     // plane size after the crop
  int tiles_y, tiles_x;
  int64_t ntiles;  // N * cgroups * tiles_y * tiles_x
  int domain;
};

// Stages the kSsimSH x kSsimSW window at (y0, x0) of `planes` planes into dst[plane][row][col]; outside the plane: 0.
// Three-channel tensors are read a whole pixel at a time when the channel is their fastest axis (channels-last).
__device__ __forceinline__ void ssim_stage(const float* __restrict__ base, SsimStrides s, const SsimJob& job, int y0, int x0,
                                           bool is_pred, float* __restrict__ dst) {
  if (job.domain == SRK_SSIM_Y8 && job.C == 3) {
    for (int i = threadIdx.x; i < kSsimPlane; i += 256) {
      const int r = i / kSsimSW, c = i - r * kSsimSW;
      float v = 0.f;
      if (y0 + r < job.H && x0 + c < job.W) {
        const float* p = base + (int64_t)(y0 + r) * s.h + (int64_t)(x0 + c) * s.w;
        v = ssim_luma(kColorDev.fwd, p[0], p[s.c], p[2 * s.c]);
      }
      dst[i] = v;
    }
    return;
  }
  const int total = job.planes * kSsimPlane;
  const bool chan_fast = job.planes > 1 && s.c < s.w;
  for (int i = threadIdx.x; i < total; i += 256) {
    int ch, pix;
    if (chan_fast) {
      pix = i / job.planes, ch = i - pix * job.planes;
    } else {
      ch = i / kSsimPlane, pix = i - ch * kSsimPlane;
    }
    const int r = pix / kSsimSW, c = pix - r * kSsimSW;
    float v = 0.f;
    if (y0 + r < job.H && x0 + c < job.W) {
      v = base[(int64_t)ch * s.c + (int64_t)(y0 + r) * s.h + (int64_t)(x0 + c) * s.w];
      if (job.domain != SRK_SSIM_FLOAT)
        v = (float)quant_u8(v);
      else if (is_pred)
        v = ssim_pred_float(v);
    }
    dst[ch * kSsimPlane + pix] = v;
  }
}

__global__ __launch_bounds__(256) void k_ssim_partial(SsimJob job, double* __restrict__ partials) {
  extern __shared__ __align__(16) unsigned char ssim_lds[];
  __shared__ double sm[4];
  float* sx = reinterpret_cast<float*>(ssim_lds);                          // [planes][SH][SW]
  float* sy = sx + job.planes * kSsimPlane;                                // [planes][SH][SW]
  double* hs = reinterpret_cast<double*>(sy + job.planes * kSsimPlane);    // [5][SH][TW]
  const int col = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int MH = job.H - kSsimHalo, MW = job.W - kSsimHalo;
  const double range = ssim_range(job.domain);
  double ssum = 0.0, qsum = 0.0;

  for (int64_t t = blockIdx.x; t < job.ntiles; t += gridDim.x) {
    int64_t u = t;
    const int tx = (int)(u % job.tiles_x);
    u /= job.tiles_x;
    const int ty = (int)(u % job.tiles_y);
    u /= job.tiles_y;
    const int cg = (int)(u % job.cgroups);
    const int64_t n = u / job.cgroups;
    const int y0 = ty * kSsimTH, x0 = tx * kSsimTW;
    ssim_stage(job.pred + n * job.ps.n + cg * job.ps.c, job.ps, job, y0, x0, true, sx);
    ssim_stage(job.gt + n * job.gs.n + cg * job.gs.c, job.gs, job, y0, x0, false, sy);
    __syncthreads();

    // squared differences of the pixels this tile owns: its own rows and columns, and the halo where it is the last tile
    const bool last_y = ty == job.tiles_y - 1, last_x = tx == job.tiles_x - 1;
    for (int i = threadIdx.x; i < job.planes * kSsimPlane; i += 256) {
      const int pix = i % kSsimPlane;
      const int r = pix / kSsimSW, c = pix - r * kSsimSW;
      if ((r < kSsimTH || last_y) && (c < kSsimTW || last_x) && y0 + r < job.H && x0 + c < job.W) {
        const double d = (double)sx[i] - (double)sy[i];
        qsum = fma(d, d, qsum);
      }
    }

    for (int p = 0; p < job.planes; ++p) {
      const float* xs = sx + p * kSsimPlane;
      const float* ys = sy + p * kSsimPlane;
      for (int r = wv; r < kSsimSH; r += 4) {   // horizontal: lane = column, conflict-free LDS reads
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < kSsimTaps; ++k) {
          const double g = kSsimWinDev.g[k];
          const double a = xs[r * kSsimSW + col + k], b = ys[r * kSsimSW + col + k];
          m[0] = fma(g, a, m[0]), m[1] = fma(g, b, m[1]);
          m[2] = fma(g, a * a, m[2]), m[3] = fma(g, b * b, m[3]), m[4] = fma(g, a * b, m[4]);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) hs[(q * kSsimSH + r) * kSsimTW + col] = m[q];
      }
      __syncthreads();
      double acc[kSsimRowsPerThread][5];
#pragma unroll
      for (int j = 0; j < kSsimRowsPerThread; ++j)
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[j][q] = 0.0;
      const int r0 = wv * kSsimRowsPerThread;
#pragma unroll
      for (int rr = 0; rr < kSsimRowsPerThread + kSsimHalo; ++rr) {   // vertical: each row sum feeds the thread's positions
        double h[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) h[q] = hs[(q * kSsimSH + r0 + rr) * kSsimTW + col];
#pragma unroll
        for (int j = 0; j < kSsimRowsPerThread; ++j) {
          const int k = rr - j;
          if (k >= 0 && k < kSsimTaps) {
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[j][q] = fma(kSsimWinDev.g[k], h[q], acc[j][q]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kSsimRowsPerThread; ++j)
        if (y0 + r0 + j < MH && x0 + col < MW)
          ssum += ssim_from_moments(acc[j][0], acc[j][1], acc[j][2], acc[j][3], acc[j][4], range);
      __syncthreads();   // hs (and after the last plane sx / sy) are written again
    }
  }
  const double s_tot = block_sum_256_d(ssum, sm);
  const double q_tot = block_sum_256_d(qsum, sm);
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = s_tot;
    partials[2 * blockIdx.x + 1] = q_tot;
  }
}

__global__ __launch_bounds__(256) void k_ssim_final(const double* __restrict__ partials, int nparts, double inv_positions,
                                                    double inv_pixels_range2, float* __restrict__ ssim_out,
                                                    float* __restrict__ psnr_out, float* __restrict__ mse_out) {
  __shared__ double sm[4];
  const double s_tot = sum_partials_256_d(partials, nparts, sm, 2);       // [block][0]: sum of the SSIM map
  const double q_tot = sum_partials_256_d(partials + 1, nparts, sm, 2);   // [block][1]: sum of squared differences
  if (threadIdx.x == 0) {
    const double mse = q_tot * inv_pixels_range2;
    *ssim_out = (float)(s_tot * inv_positions);
    if (mse_out) *mse_out = (float)mse;
    if (psnr_out) *psnr_out = (float)psnr_from_mse(mse);
  }
}

// the argument rules the device call and the host twin share
static int ssim_check(const void* pred, const void* gt, const void* ssim_out, int N, int C, int H, int W, int shave,
                      int domain, const char* who) {
  SRK_REQUIRE(pred && gt && ssim_out, "%s: null pointer", who);
  SRK_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "%s: bad dims (N %d, C %d, %d x %d)", who, N, C, H, W);
  SRK_REQUIRE(shave >= 0, "%s: negative shave (%d)", who, shave);
  SRK_REQUIRE(domain == SRK_SSIM_FLOAT || domain == SRK_SSIM_U8 || domain == SRK_SSIM_Y8, "%s: unknown domain %d", who,
              domain);
  SRK_REQUIRE(domain != SRK_SSIM_Y8 || C == 1 || C == 3, "%s: domain 'y8' takes 1 or 3 channels (got %d)", who, C);
  SRK_REQUIRE((int64_t)H - 2 * (int64_t)shave >= kSsimTaps && (int64_t)W - 2 * (int64_t)shave >= kSsimTaps,
              "%s: a plane of %d x %d with %d pixels shaved from each side is smaller than the %d x %d window", who, H, W,
              shave, kSsimTaps, kSsimTaps);
  return SRK_OK;
}

static inline SsimStrides ssim_strides(const int64_t* s, int C, int H, int W) {
  if (s) return {s[0], s[1], s[2], s[3]};
  return {(int64_t)H * W * C, 1, (int64_t)W * C, C};   // NULL: NHWC-dense, as srk_psnr
}

}  // namespace srk

using namespace srk;

extern "C" size_t srk_ssim_workspace_bytes(void) { return (size_t)kSsimPartials * 2 * sizeof(double); }

extern "C" int srk_ssim(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int N,
                        int C, int H, int W, int shave, int domain, float* ssim_out, float* psnr_out, float* mse_out,
                        void* workspace, void* stream) {
  if (int rc = ssim_check(pred, gt, ssim_out, N, C, H, W, shave, domain, "ssim")) return rc;
  SRK_REQUIRE(workspace, "ssim: null workspace");
  SsimJob job;
  job.ps = ssim_strides(pred_strides, C, H, W);
  job.gs = ssim_strides(gt_strides, C, H, W);
  job.pred = pred + shave * (job.ps.h + job.ps.w);
  job.gt = gt + shave * (job.gs.h + job.gs.w);
  job.H = H - 2 * shave, job.W = W - 2 * shave;
  const bool luma = domain == SRK_SSIM_Y8 && C == 3;
  job.cgroups = C <= kSsimMaxPlanes ? 1 : C;
  job.C = C <= kSsimMaxPlanes ? C : 1;
  job.planes = luma ? 1 : job.C;
  job.tiles_y = (int)cdiv(job.H - kSsimHalo, kSsimTH);
  job.tiles_x = (int)cdiv(job.W - kSsimHalo, kSsimTW);
  job.ntiles = (int64_t)N * job.cgroups * job.tiles_y * job.tiles_x;
  job.domain = domain;
  const int nb = (int)(job.ntiles < kSsimPartials ? job.ntiles : kSsimPartials);
  const size_t lds = (size_t)job.planes * 2 * kSsimPlane * sizeof(float) + (size_t)5 * kSsimSH * kSsimTW * sizeof(double);
  const double planes_total = (double)N * (luma ? 1 : C);
  const double range = ssim_range(domain);
  hipStream_t s = (hipStream_t)stream;
  launch_lds<&k_ssim_partial>(dim3(nb), dim3(256), lds, s, job, (double*)workspace);
  hipLaunchKernelGGL(k_ssim_final, dim3(1), dim3(256), 0, s, (const double*)workspace, nb,
                     1.0 / (planes_total * (job.H - kSsimHalo) * (double)(job.W - kSsimHalo)),
                     1.0 / (planes_total * job.H * (double)job.W * range * range), ssim_out, psnr_out, mse_out);
  return check_launch("ssim");
}

// The same definition in plain C++ double on host pointers: one plane at a time, separable, valid positions.
extern "C" int srk_ssim_host(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides,
                             int N, int C, int H, int W, int shave, int domain, double* ssim_out, double* psnr_out,
                             double* mse_out) {
  if (int rc = ssim_check(pred, gt, ssim_out, N, C, H, W, shave, domain, "ssim_host")) return rc;
  const SsimStrides ps = ssim_strides(pred_strides, C, H, W), gs = ssim_strides(gt_strides, C, H, W);
  const int h = H - 2 * shave, w = W - 2 * shave, mh = h - kSsimHalo, mw = w - kSsimHalo;
  const bool luma = domain == SRK_SSIM_Y8 && C == 3;
  const int planes = luma ? 1 : C;
  const double range = ssim_range(domain);
  const double* g = kSsimWinHost.g;
  std::vector<double> x((size_t)h * w), y((size_t)h * w), hs((size_t)5 * h * mw);
  double ssum = 0.0, qsum = 0.0;
  for (int n = 0; n < N; ++n)
    for (int p = 0; p < planes; ++p) {
      for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
          const float* pp = pred + n * ps.n + p * ps.c + (int64_t)(r + shave) * ps.h + (int64_t)(c + shave) * ps.w;
          const float* gp = gt + n * gs.n + p * gs.c + (int64_t)(r + shave) * gs.h + (int64_t)(c + shave) * gs.w;
          float a, b;
          if (luma) {
            a = ssim_luma(kColorHost.fwd, pp[0], pp[ps.c], pp[2 * ps.c]);
            b = ssim_luma(kColorHost.fwd, gp[0], gp[gs.c], gp[2 * gs.c]);
          } else if (domain != SRK_SSIM_FLOAT) {
            a = (float)quant_u8(*pp), b = (float)quant_u8(*gp);
          } else {
            a = ssim_pred_float(*pp), b = *gp;
          }
          x[(size_t)r * w + c] = a, y[(size_t)r * w + c] = b;
          const double d = (double)a - (double)b;
          qsum = fma(d, d, qsum);
        }
      for (int r = 0; r < h; ++r)
        for (int c = 0; c < mw; ++c) {
          double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
          for (int k = 0; k < kSsimTaps; ++k) {
            const double a = x[(size_t)r * w + c + k], b = y[(size_t)r * w + c + k];
            m[0] = fma(g[k], a, m[0]), m[1] = fma(g[k], b, m[1]);
            m[2] = fma(g[k], a * a, m[2]), m[3] = fma(g[k], b * b, m[3]), m[4] = fma(g[k], a * b, m[4]);
          }
          for (int q = 0; q < 5; ++q) hs[((size_t)q * h + r) * mw + c] = m[q];
        }
      for (int r = 0; r < mh; ++r)
        for (int c = 0; c < mw; ++c) {
          double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
          for (int k = 0; k < kSsimTaps; ++k)
            for (int q = 0; q < 5; ++q) m[q] = fma(g[k], hs[((size_t)q * h + r + k) * mw + c], m[q]);
          ssum += ssim_from_moments(m[0], m[1], m[2], m[3], m[4], range);
        }
    }
  const double mse = qsum / ((double)N * planes * h * (double)w * range * range);
  *ssim_out = ssum / ((double)N * planes * mh * (double)mw);
  if (mse_out) *mse_out = mse;
  if (psnr_out) *psnr_out = psnr_from_mse(mse);
  return SRK_OK;
}
