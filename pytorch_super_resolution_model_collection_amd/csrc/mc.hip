// Motion compensation for VESPCN (definitions: include/srk_mc.h and mc_common.h, shared with the host twins).
//
//   k_mc_forward<FUSE>    one thread a pixel (grid-stride): reads the flow(s), samples all C channels of the neighbour(s)
//                         bilinearly, and writes a dense NHWC tensor.  FUSE: both neighbours of frames [N,3,C,H,W] and
//                         the centre frame between them, [warp(t-1) | frame t | warp(t+1)], and the squared differences
//                         warped - centre into one double per block.  Not FUSE: one image, one flow (srk_flow_warp).
//   k_mc_finish           one block: the partials in a fixed order, the mean, the fp32 store.
//   k_mc_backward<FUSE>   one thread a pixel: recomputes the samples and writes each dflow element once,
//                         dflow = sum_c (g_c + s (warped_c - cur_c)) d warp_c / d flow,  s = seed 2 / numel [* *seed_dev].
//   k_flow_huber          loss partials and the gradient (a gather over p, p - ex, p - ey) of the smoothness term.
// The grids are functions of the sizes alone and nothing is atomic: two calls give the same bits.  Every index is built from
// clamped coordinates (mc_axis), so no flow value, NaN included, reads outside a plane.
#include "mc_common.h"
#include "srk_common.h"
#include "../../include/srk_mc.h"

namespace srk {

constexpr int kMcMaxBlocks = 1024;

static inline int mc_blocks(size_t pixels) { return (int)grid_for(pixels, 256, kMcMaxBlocks); }

struct McImages {      // the sampled image(s) and, for FUSE, the centre frame; element strides of one [N,C,H,W] view
  const float* nbr[2];
  const float* cur;
  Strides4 s;
};

template <bool FUSE>
__global__ __launch_bounds__(256) void k_mc_forward(McImages im, const float* __restrict__ flow, Strides4 fs, int N, int C,
                                                    int H, int W, float* __restrict__ out, double* __restrict__ part) {
  constexpr int K = FUSE ? 2 : 1;
  const int OC = FUSE ? 3 * C : C;
  const size_t hw = (size_t)H * W, total = (size_t)N * hw;
  double acc = 0.0;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (size_t)gridDim.x * 256) {
    const int n = (int)(p / hw), r = (int)(p % hw), y = r / W, x = r % W;
    float* o = out + p * OC;
    const float* cur = FUSE ? im.cur + n * im.s.n + y * im.s.h + x * im.s.w : nullptr;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float* f = flow + (int64_t)(n + k * N) * fs.n + y * fs.h + x * fs.w;
      const McTap<float> t = mc_tap<float>(f[0], f[fs.c], x, y, H, W);
      const float* img = im.nbr[k] + n * im.s.n;
      for (int c = 0; c < C; ++c) {
        const float v = mc_sample<float>(img + c * im.s.c, im.s.h, im.s.w, t, nullptr, nullptr);
        o[k * 2 * C + c] = v;
        if (FUSE) {
          const double d = (double)v - (double)cur[c * im.s.c];
          acc += d * d;
        }
      }
    }
    if (FUSE)
      for (int c = 0; c < C; ++c) o[C + c] = cur[c * im.s.c];
  }
  if constexpr (FUSE) {
    __shared__ double sm[4];
    store_block_sum_256_d(acc, sm, part + blockIdx.x);
  }
}

__global__ __launch_bounds__(256) void k_mc_finish(const double* __restrict__ part, int nparts, double inv_n,
                                                   float* __restrict__ loss) {
  __shared__ double sm[4];
  const double tot = sum_partials_256_d(part, nparts, sm);
  if (threadIdx.x == 0) *loss = (float)(tot * inv_n);
}

template <bool FUSE>
__global__ __launch_bounds__(256) void k_mc_backward(McImages im, const float* __restrict__ flow, Strides4 fs,
                                                     const float* __restrict__ g, Strides4 gs, int N, int C, int H, int W,
                                                     float s, const float* __restrict__ seed_dev, float* __restrict__ dflow,
                                                     Strides4 ds) {
  constexpr int K = FUSE ? 2 : 1;
  const size_t hw = (size_t)H * W, total = (size_t)N * hw;
  if (FUSE && seed_dev) s *= *seed_dev;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (size_t)gridDim.x * 256) {
    const int n = (int)(p / hw), r = (int)(p % hw), y = r / W, x = r % W;
    const float* cur = FUSE ? im.cur + n * im.s.n + y * im.s.h + x * im.s.w : nullptr;
    const float* gp = g ? g + n * gs.n + y * gs.h + x * gs.w : nullptr;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float* f = flow + (int64_t)(n + k * N) * fs.n + y * fs.h + x * fs.w;
      const McTap<float> t = mc_tap<float>(f[0], f[fs.c], x, y, H, W);
      const float* img = im.nbr[k] + n * im.s.n;
      float ax = 0.f, ay = 0.f;
      for (int c = 0; c < C; ++c) {
        float dvx, dvy;
        const float v = mc_sample<float>(img + c * im.s.c, im.s.h, im.s.w, t, &dvx, &dvy);
        float up = gp ? gp[(k * 2 * C + c) * gs.c] : 0.f;
        if (FUSE) up += s * (v - cur[c * im.s.c]);
        ax += up * dvx;
        ay += up * dvy;
      }
      float* d = dflow + (int64_t)(n + k * N) * ds.n + y * ds.h + x * ds.w;
      d[0] = ax;
      d[ds.c] = ay;
    }
  }
}

__global__ __launch_bounds__(256) void k_flow_huber(const float* __restrict__ flow, Strides4 fs, int M, int H, int W,
                                                    double eps, double scale_over_n, float* __restrict__ dflow,
                                                    double* __restrict__ part) {
  __shared__ double sm[4];
  const size_t hw = (size_t)H * W, total = (size_t)M * hw;
  double acc = 0.0;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (size_t)gridDim.x * 256) {
    const int m = (int)(p / hw), r = (int)(p % hw), y = r / W, x = r % W;
    const float* f = flow + m * fs.n;
    double h, gu, gv;
    if (dflow) {
      huber_grad_at(f, fs.c, fs.h, fs.w, y, x, H, W, eps, &h, &gu, &gv);
      float* d = dflow + m * fs.n + y * fs.h + x * fs.w;     // the gradient is stored like the flow
      d[0] = (float)(scale_over_n * gu);
      d[fs.c] = (float)(scale_over_n * gv);
    } else {
      double e[4];
      h = huber_at(f, fs.c, fs.h, fs.w, y, x, H, W, eps, e);
    }
    acc += h;
  }
  store_block_sum_256_d(acc, sm, part + blockIdx.x);
}

// ---- what the device entry points and the host twins check alike ----
static int mc_ok(const char* who, const void* img, const void* flow, const int64_t* is, const int64_t* fs, int N, int C, int H,
                 int W) {
  SRK_REQUIRE(img && flow && fs, "%s: null pointer", who);
  SRK_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: non-positive size N %d C %d H %d W %d", who, N, C, H, W);
  SRK_REQUIRE((int64_t)H * W <= INT32_MAX && (int64_t)C * 3 <= INT32_MAX / 2, "%s: a plane of %d x %d or %d channels is too large",
              who, H, W, C);
  for (int i = 0; i < 4; ++i) {
    SRK_REQUIRE(fs[i] >= 0, "%s: negative flow stride %lld", who, (long long)fs[i]);
    SRK_REQUIRE(!is || is[i] >= 0, "%s: negative image stride %lld", who, (long long)is[i]);
  }
  return SRK_OK;
}

static McImages mc_frames(const float* frames, int C, int H, int W) {
  const int64_t hw = (int64_t)H * W;
  return McImages{{frames, frames + 2 * C * hw}, frames + C * hw, Strides4{3 * C * hw, hw, W, 1}};
}

template <bool FUSE>
static void mc_host(const McImages& im, const float* flow, Strides4 fs, int N, int C, int H, int W, double seed, const double* g,
                    double* out, double* loss, double* dflow) {
  constexpr int K = FUSE ? 2 : 1;
  const int OC = FUSE ? 3 * C : C;
  const int64_t hw = (int64_t)H * W;
  const double s = FUSE ? seed * 2.0 / ((double)K * N * C * (double)hw) : 0.0;
  double acc = 0.0;
  for (int n = 0; n < N; ++n)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const float* cur = FUSE ? im.cur + n * im.s.n + y * im.s.h + x * im.s.w : nullptr;
        const int64_t px = (int64_t)y * W + x;
        for (int k = 0; k < K; ++k) {
          const float* f = flow + (int64_t)(n + k * N) * fs.n + y * fs.h + x * fs.w;
          const McTap<double> t = mc_tap<double>((double)f[0], (double)f[fs.c], x, y, H, W);
          double ax = 0.0, ay = 0.0;
          for (int c = 0; c < C; ++c) {
            double dvx, dvy;
            const double v = mc_sample<double>(im.nbr[k] + n * im.s.n + c * im.s.c, im.s.h, im.s.w, t, &dvx, &dvy);
            const int64_t oi = ((int64_t)n * OC + k * 2 * C + c) * hw + px;
            out[oi] = v;
            double up = g ? g[oi] : 0.0;
            if (FUSE) {
              const double d = v - (double)cur[c * im.s.c];
              acc += d * d;
              up += s * d;
            }
            ax += up * dvx;
            ay += up * dvy;
          }
          if (dflow) {
            dflow[((int64_t)(n + k * N) * 2 + 0) * hw + px] = ax;
            dflow[((int64_t)(n + k * N) * 2 + 1) * hw + px] = ay;
          }
        }
        if (FUSE)
          for (int c = 0; c < C; ++c) out[((int64_t)n * OC + C + c) * hw + px] = (double)cur[c * im.s.c];
      }
  if (FUSE) *loss = acc / ((double)K * N * C * (double)hw);
}

}  // namespace srk

using namespace srk;

extern "C" size_t srk_mc_workspace_bytes(void) { return (size_t)kMcMaxBlocks * sizeof(double); }

extern "C" int srk_motion_fuse_forward(const float* frames, const float* flow, const int64_t* flow_strides, int N, int C, int H,
                                       int W, float* fused, float* mc_loss, void* workspace, void* stream) {
  const char* who = "motion_fuse_forward";
  if (int rc = mc_ok(who, frames, flow, nullptr, flow_strides, N, C, H, W)) return rc;
  SRK_REQUIRE(fused && mc_loss && workspace, "%s: null pointer", who);
  SRK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: workspace is not 8-byte aligned", who);
  const size_t pixels = (size_t)N * H * W;
  const int nb = mc_blocks(pixels);
  double* part = reinterpret_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mc_forward<true>, dim3(nb), dim3(256), 0, s, mc_frames(frames, C, H, W), flow, strides4(flow_strides), N,
                     C, H, W, fused, part);
  hipLaunchKernelGGL(k_mc_finish, dim3(1), dim3(256), 0, s, (const double*)part, nb, 1.0 / (2.0 * C * (double)pixels), mc_loss);
  return check_launch(who);
}

extern "C" int srk_motion_fuse_backward(const float* frames, const float* flow, const int64_t* flow_strides, const float* g_fused,
                                        const int64_t* g_strides, int N, int C, int H, int W, float seed, const float* seed_dev,
                                        float* dflow, const int64_t* dflow_strides, void* stream) {
  const char* who = "motion_fuse_backward";
  if (int rc = mc_ok(who, frames, flow, nullptr, flow_strides, N, C, H, W)) return rc;
  SRK_REQUIRE(dflow && dflow_strides && (!g_fused || g_strides), "%s: null pointer", who);
  for (int i = 0; i < 4; ++i)
    SRK_REQUIRE(dflow_strides[i] >= 0 && (!g_fused || g_strides[i] >= 0), "%s: negative stride", who);
  const size_t pixels = (size_t)N * H * W;
  const Strides4 gs = g_fused ? strides4(g_strides) : Strides4{0, 0, 0, 0};
  const float sc = (float)((double)seed * 2.0 / (2.0 * C * (double)pixels));
  hipLaunchKernelGGL(k_mc_backward<true>, dim3(mc_blocks(pixels)), dim3(256), 0, (hipStream_t)stream,
                     mc_frames(frames, C, H, W), flow, strides4(flow_strides), g_fused, gs, N, C, H, W, sc, seed_dev, dflow,
                     strides4(dflow_strides));
  return check_launch(who);
}

extern "C" int srk_flow_warp_forward(const float* img, const int64_t* img_strides, const float* flow, const int64_t* flow_strides,
                                     int N, int C, int H, int W, float* out, void* stream) {
  const char* who = "flow_warp_forward";
  SRK_REQUIRE(img_strides && out, "%s: null pointer", who);
  if (int rc = mc_ok(who, img, flow, img_strides, flow_strides, N, C, H, W)) return rc;
  const size_t pixels = (size_t)N * H * W;
  hipLaunchKernelGGL(k_mc_forward<false>, dim3(mc_blocks(pixels)), dim3(256), 0, (hipStream_t)stream,
                     McImages{{img, nullptr}, nullptr, strides4(img_strides)}, flow, strides4(flow_strides), N, C, H, W, out,
                     (double*)nullptr);
  return check_launch(who);
}

extern "C" int srk_flow_warp_backward(const float* img, const int64_t* img_strides, const float* flow, const int64_t* flow_strides,
                                      const float* g, const int64_t* g_strides, int N, int C, int H, int W, float* dflow,
                                      const int64_t* dflow_strides, void* stream) {
  const char* who = "flow_warp_backward";
  SRK_REQUIRE(img_strides && g && g_strides && dflow && dflow_strides, "%s: null pointer", who);
  if (int rc = mc_ok(who, img, flow, img_strides, flow_strides, N, C, H, W)) return rc;
  for (int i = 0; i < 4; ++i) SRK_REQUIRE(dflow_strides[i] >= 0 && g_strides[i] >= 0, "%s: negative stride", who);
  const size_t pixels = (size_t)N * H * W;
  hipLaunchKernelGGL(k_mc_backward<false>, dim3(mc_blocks(pixels)), dim3(256), 0, (hipStream_t)stream,
                     McImages{{img, nullptr}, nullptr, strides4(img_strides)}, flow, strides4(flow_strides), g,
                     strides4(g_strides), N, C, H, W, 0.f, (const float*)nullptr, dflow, strides4(dflow_strides));
  return check_launch(who);
}

static int huber_ok(const char* who, const void* flow, const int64_t* fs, int M, int H, int W, double eps) {
  SRK_REQUIRE(flow && fs, "%s: null pointer", who);
  SRK_REQUIRE(M >= 1 && H >= 1 && W >= 1, "%s: non-positive size M %d H %d W %d", who, M, H, W);
  SRK_REQUIRE((int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d is too large", who, H, W);
  SRK_REQUIRE(eps > 0.0, "%s: eps %g is not positive", who, eps);
  for (int i = 0; i < 4; ++i) SRK_REQUIRE(fs[i] >= 0, "%s: negative flow stride %lld", who, (long long)fs[i]);
  return SRK_OK;
}

extern "C" int srk_flow_huber_forward_backward(const float* flow, const int64_t* flow_strides, int M, int H, int W, float eps,
                                               float grad_scale, float* loss, float* dflow, void* workspace, void* stream) {
  const char* who = "flow_huber_forward_backward";
  if (int rc = huber_ok(who, flow, flow_strides, M, H, W, (double)eps)) return rc;
  SRK_REQUIRE(loss && workspace, "%s: null pointer", who);
  SRK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: workspace is not 8-byte aligned", who);
  const size_t pixels = (size_t)M * H * W;
  const int nb = mc_blocks(pixels);
  double* part = reinterpret_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_flow_huber, dim3(nb), dim3(256), 0, s, flow, strides4(flow_strides), M, H, W, (double)eps,
                     (double)grad_scale / (double)pixels, dflow, part);
  hipLaunchKernelGGL(k_mc_finish, dim3(1), dim3(256), 0, s, (const double*)part, nb, 1.0 / (double)pixels, loss);
  return check_launch(who);
}

extern "C" int srk_motion_fuse_host(const float* frames, const float* flow, const int64_t* flow_strides, int N, int C, int H,
                                    int W, double seed, const double* g_fused, double* fused, double* mc_loss, double* dflow) {
  const char* who = "motion_fuse_host";
  if (int rc = mc_ok(who, frames, flow, nullptr, flow_strides, N, C, H, W)) return rc;
  SRK_REQUIRE(fused && mc_loss, "%s: null pointer", who);
  mc_host<true>(mc_frames(frames, C, H, W), flow, strides4(flow_strides), N, C, H, W, seed, g_fused, fused, mc_loss, dflow);
  return SRK_OK;
}

extern "C" int srk_flow_warp_host(const float* img, const int64_t* img_strides, const float* flow, const int64_t* flow_strides,
                                  int N, int C, int H, int W, const double* g, double* out, double* dflow) {
  const char* who = "flow_warp_host";
  SRK_REQUIRE(img_strides && out, "%s: null pointer", who);
  if (int rc = mc_ok(who, img, flow, img_strides, flow_strides, N, C, H, W)) return rc;
  mc_host<false>(McImages{{img, nullptr}, nullptr, strides4(img_strides)}, flow, strides4(flow_strides), N, C, H, W, 0.0, g, out,
                 nullptr, dflow);
  return SRK_OK;
}

extern "C" int srk_flow_huber_host(const float* flow, const int64_t* flow_strides, int M, int H, int W, double eps,
                                   double grad_scale, double* loss, double* dflow) {
  const char* who = "flow_huber_host";
  if (int rc = huber_ok(who, flow, flow_strides, M, H, W, eps)) return rc;
  SRK_REQUIRE(loss, "%s: null pointer", who);
  const Strides4 fs = strides4(flow_strides);
  const int64_t hw = (int64_t)H * W;
  const double scale_over_n = grad_scale / ((double)M * (double)hw);
  double acc = 0.0;
  for (int m = 0; m < M; ++m)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        double h, gu, gv;
        huber_grad_at(flow + m * fs.n, fs.c, fs.h, fs.w, y, x, H, W, eps, &h, &gu, &gv);
        acc += h;
        if (dflow) {      // dense [M][2][H][W]
          dflow[((int64_t)m * 2 + 0) * hw + (int64_t)y * W + x] = scale_over_n * gu;
          dflow[((int64_t)m * 2 + 1) * hw + (int64_t)y * W + x] = scale_over_n * gv;
        }
      }
  *loss = acc / ((double)M * (double)hw);
  return SRK_OK;
}
