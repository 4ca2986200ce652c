// Steps either side of the nets that the reference runs on the host every iteration / every test image
// (SURVEY.md §8 f2, a5): PSNR (utils.py:208-216), norm / denorm (utils.py:219-239), the nearest x2 resize of
// Upsample2xBlock('rnc') (base_networks.py:204-210), the 2x2 max-pool of the VGG19 feature extractor
// (srgan.py:84-90) and per-sample statistics for norm='instance' (base_networks.py:48,83,119,163).
// All HBM-bound streaming kernels; grid-stride loops, 16-byte accesses where the layout allows.
#include "srk_common.h"

namespace srk {

constexpr int kPsnrPartials = 1024;

constexpr int kPpMaxBlocks = 4096;   // grid cap of every kernel here

// ---------------------------------------------------------------------------------------------
// PSNR: mse = mean((clamp(pred,0,1) - gt)^2); psnr = mse == 0 ? 100 : 10*log10(1/mse).  pred is addressed
// NHWC-dense or through element strides like the target (a net output is channels_last, a loader's target NCHW).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_psnr_partial(const float* __restrict__ pred, Strides4 ps,
                                                      const float* __restrict__ gt, Strides4 gs, int C, int H, int W,
                                                      size_t total, double* __restrict__ partials) {
  __shared__ double sm[4];
  double acc = 0.0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    // e enumerates (n, h, w, c) with c fastest
    const int c = (int)(e % C);
    size_t t = e / C;
    const int w = (int)(t % W);
    t /= W;
    const int h = (int)(t % H);
    const int64_t n = (int64_t)(t / H);
    float p = pred[n * ps.n + c * ps.c + h * ps.h + w * ps.w];
    p = fminf(fmaxf(p, 0.f), 1.f);
    const float d = p - gt[n * gs.n + c * gs.c + h * gs.h + w * gs.w];  // fp32 difference, as the reference
    acc += (double)d * (double)d;
  }
  store_block_sum_256_d(acc, sm, partials + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_psnr_final(const double* __restrict__ partials, int nparts, double inv_count,
                                                    float* __restrict__ psnr, float* __restrict__ mse_out) {
  __shared__ double sm[4];
  const double tot = sum_partials_256_d(partials, nparts, sm);
  if (threadIdx.x == 0) {
    const double mse = tot * inv_count;
    if (mse_out) *mse_out = (float)mse;
    *psnr = mse == 0.0 ? 100.f : (float)(10.0 * log10(1.0 / mse));
  }
}

// ---------------------------------------------------------------------------------------------
// y = (x - sub[c]) / div[c], optionally clamped to [0,1].  torchvision.transforms.Normalize is
// tensor.sub_(mean).div_(std) in fp32: the same two IEEE operations here, so results are bit-equal.
// channel of element e = (e / inner) % C  (inner = H*W for NCHW storage, 1 for NHWC storage).
// ---------------------------------------------------------------------------------------------
struct AffineConsts {
  float sub[8], div[8];
};

__global__ __launch_bounds__(256) void k_channel_affine(const float* __restrict__ x, float* __restrict__ y, size_t total,
                                                        int C, size_t inner, AffineConsts k, int clamp01) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int c = (int)((e / inner) % C);
    float v = (x[e] - k.sub[c]) / k.div[c];
    if (clamp01) v = fminf(fmaxf(v, 0.f), 1.f);
    y[e] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// Nearest-neighbour integer up-sampling, NHWC: y[n, oy, ox, c] = x[n, oy / r, ox / r, c]
// (torch.nn.Upsample(scale_factor=r, mode='nearest')); backward sums each r x r block.
// ---------------------------------------------------------------------------------------------
// V = 4 (C % 4 == 0): one 16-byte group of channels per thread and pass; CG = C / V.
template <int V>
__global__ __launch_bounds__(256) void k_upsample_nearest_fwd(const float* __restrict__ x, float* __restrict__ y, int H,
                                                              int W, int CG, int r, size_t groups) {
  typedef Vec<V> Q;
  const int OW = W * r, OH = H * r;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < groups; e += (size_t)gridDim.x * 256) {
    const int c = (int)(e % CG);
    size_t t = e / CG;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH);
    const size_t n = t / OH;
    Q::store(y, e, Q::load(x, ((n * H + oy / r) * W + ox / r) * CG + c));
  }
}

__global__ __launch_bounds__(256) void k_upsample_nearest_bwd(const float* __restrict__ dy, float* __restrict__ dx,
                                                              int H, int W, int C, int r, size_t total) {
  const int OW = W * r;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    size_t t = e / C;
    const int xx = (int)(t % W);
    t /= W;
    const int yy = (int)(t % H);
    const size_t n = t / H;
    float acc = 0.f;
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < r; ++j) acc += dy[((n * H * r + (size_t)yy * r + i) * OW + (size_t)xx * r + j) * C + c];
    dx[e] = acc;
  }
}

// ---------------------------------------------------------------------------------------------
// MaxPool2d(kernel 2, stride 2), NHWC, floor mode (odd trailing row / column dropped) — vgg19.features[4].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_maxpool2(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C,
                                                  size_t total) {
  const int OH = H / 2, OW = W / 2;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    size_t t = e / C;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH);
    const size_t n = t / OH;
    const float* p = x + ((n * H + (size_t)oy * 2) * W + (size_t)ox * 2) * C + c;
    const float a = p[0], b = p[C], d = p[(size_t)W * C], f = p[(size_t)W * C + C];
    // NaN-propagating like ATen's max_pool2d: a NaN anywhere in the window wins
    float m = a;
    if (b > m || b != b) m = b;
    if (d > m || d != d) m = d;
    if (f > m || f != f) m = f;
    y[e] = m;
  }
}

// ---------------------------------------------------------------------------------------------
// Gradient of that pool.  No index tensor is saved: the winner of a window is recomputed from x, as the conv kernels
// recompute their masks.  The winner is ATen's: the FIRST maximum in (row, column) scan order, i.e. only a strictly
// greater value replaces the running one.  NaN inputs are out of scope here (the forward propagates a NaN; a window
// holding one routes its gradient to whichever element the comparisons above leave).
// One thread owns one 2x2 window of V channels and writes all four dx elements of it; the grid of windows is
// ceil(H/2) x ceil(W/2), so with odd H / W the partial windows of the trailing row / column are owned too and get their
// zeros: every dx element is written exactly once, no memset, no atomics.  The five loads are unconditional, from
// addresses clamped into the tensors, and the values are selected afterwards (a load under a divergent branch costs a
// full vmcnt(0) wait at the join).
// relu_input: x is the output of a fused conv + ReLU whose backward would multiply this dx by (x > 0).  A window whose
// maximum is <= 0 then routes nothing (its winner is a zero, masked below anyway; a positive winner passes the mask
// unchanged), so dx leaves pre-masked and the conv below skips its mask read (ops.PREMASK).
// ---------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void k_maxpool2_bwd(const float* __restrict__ x, const float* __restrict__ dy,
                                                      float* __restrict__ dx, int H, int W, int C, int relu_input,
                                                      size_t total) {
  typedef Vec<V> Q;
  const int OH = H / 2, OW = W / 2, WH = (H + 1) / 2, WW = (W + 1) / 2, CG = C / V;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int cg = (int)(e % CG);
    size_t t = e / CG;
    const int wx = (int)(t % WW);
    t /= WW;
    const int wy = (int)(t % WH);
    const size_t n = t / WH;
    const int y0 = 2 * wy, x0 = 2 * wx;   // always inside the plane
    const bool has_y1 = y0 + 1 < H, has_x1 = x0 + 1 < W;
    const bool window = has_y1 && has_x1;   // a whole window: the pool has an output here
    const int y1 = has_y1 ? y0 + 1 : y0, x1 = has_x1 ? x0 + 1 : x0;   // clamped: loads stay inside x
    const int py = wy < OH ? wy : OH - 1, px = wx < OW ? wx : OW - 1;   // ... and inside dy
    const size_t c0 = (size_t)cg * V;
    const size_t r0 = (n * H + y0) * W, r1 = (n * H + y1) * W;
    const size_t i00 = (r0 + x0) * C + c0, i01 = (r0 + x1) * C + c0, i10 = (r1 + x0) * C + c0, i11 = (r1 + x1) * C + c0;
    // (every index below is a multiple of V floats: C % V == 0)
    const typename Q::T a = Q::load(x + i00, 0), b = Q::load(x + i01, 0), d = Q::load(x + i10, 0), f = Q::load(x + i11, 0);
    const typename Q::T g = Q::load(dy + ((n * OH + py) * OW + px) * C + c0, 0);
    typename Q::T o0, o1, o2, o3;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float m = Q::at(a, i);
      int k = 0;
      if (Q::at(b, i) > m) m = Q::at(b, i), k = 1;
      if (Q::at(d, i) > m) m = Q::at(d, i), k = 2;
      if (Q::at(f, i) > m) m = Q::at(f, i), k = 3;
      const bool route = window && !(relu_input && m <= 0.f);
      const float gi = route ? Q::at(g, i) : 0.f;
      Q::set(o0, i, k == 0 ? gi : 0.f);
      Q::set(o1, i, k == 1 ? gi : 0.f);
      Q::set(o2, i, k == 2 ? gi : 0.f);
      Q::set(o3, i, k == 3 ? gi : 0.f);
    }
    Q::store(dx + i00, 0, o0);
    if (has_x1) Q::store(dx + i01, 0, o1);
    if (has_y1) {
      Q::store(dx + i10, 0, o2);
      if (has_x1) Q::store(dx + i11, 0, o3);
    }
  }
}

}  // namespace srk

using namespace srk;

extern "C" size_t srk_psnr_workspace_bytes(void) { return kPsnrPartials * sizeof(double); }

extern "C" int srk_psnr(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int N,
                        int C, int H, int W, float* psnr_out, float* mse_out, void* workspace, void* stream) {
  SRK_REQUIRE(pred && gt && psnr_out && workspace, "psnr: null pointer");
  SRK_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "psnr: bad dims");
  const Strides4 dense = {(int64_t)H * W * C, 1, (int64_t)W * C, C};
  Strides4 ps = dense, gs = dense;
  if (pred_strides) ps = strides4(pred_strides);
  if (gt_strides) gs = strides4(gt_strides);
  const size_t total = (size_t)N * C * H * W;
  unsigned nb = grid_for(total, 256 * 8, kPpMaxBlocks);
  if (nb > kPsnrPartials) nb = kPsnrPartials;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_psnr_partial, dim3(nb), dim3(256), 0, s, pred, ps, gt, gs, C, H, W, total, (double*)workspace);
  hipLaunchKernelGGL(k_psnr_final, dim3(1), dim3(256), 0, s, (const double*)workspace, (int)nb, 1.0 / (double)total,
                     psnr_out, mse_out);
  return check_launch("psnr");
}

extern "C" int srk_channel_affine(const float* x, float* y, size_t n, int C, size_t inner, const float* sub_host,
                                  const float* div_host, int clamp01, void* stream) {
  SRK_REQUIRE(x && y && sub_host && div_host && n > 0, "channel_affine: null pointer or empty");
  SRK_REQUIRE(C >= 1 && C <= 8 && inner >= 1, "channel_affine: 1..8 channels supported (got %d)", C);
  AffineConsts k;
  for (int c = 0; c < 8; ++c) {
    k.sub[c] = c < C ? sub_host[c] : 0.f;
    k.div[c] = c < C ? div_host[c] : 1.f;
    SRK_REQUIRE(k.div[c] != 0.f, "channel_affine: zero divisor for channel %d", c);
  }
  hipLaunchKernelGGL(k_channel_affine, dim3(grid_for(n, 256 * 4, kPpMaxBlocks)), dim3(256), 0, (hipStream_t)stream, x,
                     y, n, C, inner, k, clamp01);
  return check_launch("channel_affine");
}

extern "C" int srk_upsample_nearest_forward(const float* x, float* y, int N, int H, int W, int C, int r, void* stream) {
  SRK_REQUIRE(x && y, "upsample_nearest: null pointer");
  SRK_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && r >= 1, "upsample_nearest: bad dims");
  const size_t total = (size_t)N * H * r * W * r * C;
  hipStream_t s = (hipStream_t)stream;
  if (C % 4 == 0)
    hipLaunchKernelGGL(k_upsample_nearest_fwd<4>, dim3(grid_for(total / 4, 256 * 2, kPpMaxBlocks)), dim3(256), 0, s, x,
                       y, H, W, C / 4, r, total / 4);
  else
    hipLaunchKernelGGL(k_upsample_nearest_fwd<1>, dim3(grid_for(total, 256 * 4, kPpMaxBlocks)), dim3(256), 0, s, x, y,
                       H, W, C, r, total);
  return check_launch("upsample_nearest_forward");
}

extern "C" int srk_upsample_nearest_backward(const float* dy, float* dx, int N, int H, int W, int C, int r,
                                             void* stream) {
  SRK_REQUIRE(dy && dx, "upsample_nearest_backward: null pointer");
  SRK_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && r >= 1, "upsample_nearest_backward: bad dims");
  const size_t total = (size_t)N * H * W * C;
  hipLaunchKernelGGL(k_upsample_nearest_bwd, dim3(grid_for(total, 256 * 2, kPpMaxBlocks)), dim3(256), 0,
                     (hipStream_t)stream, dy, dx, H, W, C, r, total);
  return check_launch("upsample_nearest_backward");
}

extern "C" int srk_maxpool2x2_forward(const float* x, float* y, int N, int H, int W, int C, void* stream) {
  SRK_REQUIRE(x && y, "maxpool2x2: null pointer");
  SRK_REQUIRE(N > 0 && H >= 2 && W >= 2 && C > 0, "maxpool2x2: bad dims");
  const size_t total = (size_t)N * (H / 2) * (W / 2) * C;
  hipLaunchKernelGGL(k_maxpool2, dim3(grid_for(total, 256 * 4, kPpMaxBlocks)), dim3(256), 0, (hipStream_t)stream, x, y,
                     H, W, C, total);
  return check_launch("maxpool2x2_forward");
}

extern "C" int srk_maxpool2x2_backward(const float* x, const float* dy, float* dx, int N, int H, int W, int C,
                                       int relu_input, void* stream) {
  SRK_REQUIRE(x && dy && dx, "maxpool2x2_backward: null pointer");
  SRK_REQUIRE(N > 0 && H >= 2 && W >= 2 && C > 0, "maxpool2x2_backward: bad dims");
  const size_t windows = (size_t)N * ((H + 1) / 2) * ((W + 1) / 2);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = C % 4 == 0 && aligned16(x, dy, dx);
  const size_t total = vec ? windows * (C / 4) : windows * C;
  const unsigned nb = vec ? grid_for(total, 256, kPpMaxBlocks) : grid_for(total, 256 * 2, kPpMaxBlocks);
  hipLaunchKernelGGL(vec ? k_maxpool2_bwd<4> : k_maxpool2_bwd<1>, dim3(nb), dim3(256), 0, s, x, dy, dx, H, W, C,
                     relu_input != 0, total);
  return check_launch("maxpool2x2_backward");
}
