// Real-ESRGAN's USMSharp on the loader's 8-bit patches (data.py: usm=True; include/srk.h), defined to the
// byte: fp64 sums in a fixed tap order, nothing contracted, so a numpy restatement gives the same bytes.
//
//   Bl = blur(P);  R = P - Bl;  M = |R| > threshold;  S = blur(M);  y = round(S * clamp(P + weight * R) + (1 - S) * P)
//
// blur is the separable Gaussian g[K] (K odd <= 51), rows then columns, borders reflect-101.  Both blurs read bytes (P, then
// the 0 / 1 mask), so ONE kernel body serves both: k_usm_pass<false> makes R and M, k_usm_pass<true> makes S and the result.
// A block owns kUsmTH x kUsmTW outputs of one plane.  It stages them plus the halo of K / 2 as bytes in LDS (6.9 KB) with
// the table beside them, runs the row pass over the TH + K - 1 staged rows into an fp64 LDS tile (21 KB) and the column
// pass out of that tile: the unrounded intermediate never leaves the CU.  The halo rows are blurred again by the blocks
// above and below ((TH + K - 1) / TH = 2.6 times the row work at K = 51): patch-sized planes are a few tiles, and the
// alternative is an fp64 round trip through HBM per pass.  28.3 KB of LDS a block, five blocks a CU.
#include "srk_common.h"
#include "usm_common.h"
#include <vector>

namespace srk {

constexpr int kUsmTH = 32, kUsmTW = 32;
constexpr int kUsmSH = kUsmTH + kUsmMaxK - 1;                  // staged rows at the widest table
constexpr int kUsmPitch = (kUsmTW + kUsmMaxK - 1 + 3) & ~3;    // bytes per staged row
static_assert(kUsmTH * kUsmTW % 256 == 0, "256 threads share the tile's outputs evenly");

template <bool kSecond>
__global__ __launch_bounds__(256) void k_usm_pass(const uint8_t* __restrict__ x, const uint8_t* __restrict__ src,
                                                  const double* __restrict__ g, int K, double weight, double threshold,
                                                  double* __restrict__ R, uint8_t* __restrict__ M, uint8_t* __restrict__ y,
                                                  int H, int W, int tiles_x, int tiles_per_plane) {
  __shared__ double sg[kUsmMaxK];
  __shared__ double srow[kUsmSH * kUsmTW];
  __shared__ uint8_t sb[kUsmSH * kUsmPitch];
  const int r0 = K / 2, SH = kUsmTH + K - 1, SW = kUsmTW + K - 1;
  const int plane = blockIdx.x / tiles_per_plane, t = blockIdx.x - plane * tiles_per_plane;
  const int ty0 = (t / tiles_x) * kUsmTH, tx0 = (t % tiles_x) * kUsmTW;
  const size_t base = (size_t)plane * H * W;
  const uint8_t* __restrict__ sp = src + base;
  for (int i = threadIdx.x; i < K; i += 256) sg[i] = g[i];
  for (int i = threadIdx.x; i < SH * SW; i += 256) {
    const int r = i / SW, c = i - r * SW;
    sb[r * kUsmPitch + c] = sp[(size_t)usm_reflect(ty0 + r - r0, H, r0) * W + usm_reflect(tx0 + c - r0, W, r0)];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SH * kUsmTW; i += 256) {
    const int r = i / kUsmTW, c = i - r * kUsmTW;
    srow[i] = usm_taps(sg, sb + r * kUsmPitch + c, 1, K);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kUsmTH * kUsmTW; i += 256) {
    const int r = i / kUsmTW, c = i - r * kUsmTW;
    const int oy = ty0 + r, ox = tx0 + c;
    if (oy >= H || ox >= W) continue;
    const double v = usm_taps(sg, srow + i, kUsmTW, K);
    const size_t e = base + (size_t)oy * W + ox;
    if constexpr (kSecond) {
      y[e] = usm_finish(x[e], R[e], v, weight);
    } else {
      usm_residual(x[e], v, threshold, R + e, M + e);
    }
  }
}

static size_t usm_align256(size_t v) { return (v + 255) & ~(size_t)255; }

static int usm_check(const char* what, const void* x, const void* y, const double* g, int K, int B, int C, int H, int W) {
  SRK_REQUIRE(x && y && g, "%s: null pointer", what);
  SRK_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad dims (B %d, %d x %d)", what, B, H, W);
  SRK_REQUIRE(C == 1 || C == 3, "%s: C must be 1 or 3 (got %d)", what, C);
  SRK_REQUIRE(K >= 1 && K <= kUsmMaxK && (K & 1), "%s: K must be odd and in [1, %d] (got %d)", what, kUsmMaxK, K);
  SRK_REQUIRE(H > K / 2 && W > K / 2, "%s: a %d x %d plane cannot mirror a halo of %d (reflect-101 needs H, W > K / 2)", what,
              H, W, K / 2);
  return SRK_OK;
}

}  // namespace srk

using namespace srk;

extern "C" size_t srk_usm_u8_workspace_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  const size_t n = (size_t)B * C * H * W;
  return usm_align256(n * sizeof(double)) + usm_align256(n);
}

extern "C" int srk_usm_u8(const uint8_t* x, uint8_t* y, const double* g, int K, double weight, double threshold, int B, int C,
                          int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = usm_check("usm_u8", x, y, g, K, B, C, H, W)) return rc;
  const size_t need = srk_usm_u8_workspace_bytes(B, C, H, W);
  if (!workspace || workspace_bytes < need) {
    set_error("usm_u8: workspace %zu < %zu", workspace_bytes, need);
    return SRK_ERR_WORKSPACE;
  }
  const int tiles_x = (W + kUsmTW - 1) / kUsmTW, tiles_y = (H + kUsmTH - 1) / kUsmTH, tpp = tiles_x * tiles_y;
  const int64_t blocks = (int64_t)B * C * tpp;
  SRK_REQUIRE(blocks <= 0x7fffffff, "usm_u8: %lld tiles are more than one launch takes", (long long)blocks);
  const size_t n = (size_t)B * C * H * W;
  double* R = static_cast<double*>(workspace);
  uint8_t* M = reinterpret_cast<uint8_t*>(static_cast<char*>(workspace) + usm_align256(n * sizeof(double)));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_usm_pass<false>, dim3((unsigned)blocks), dim3(256), 0, s, x, x, g, K, weight, threshold, R, M, y, H, W,
                     tiles_x, tpp);
  hipLaunchKernelGGL(k_usm_pass<true>, dim3((unsigned)blocks), dim3(256), 0, s, x, (const uint8_t*)M, g, K, weight, threshold,
                     R, M, y, H, W, tiles_x, tpp);
  return check_launch("usm_u8");
}

extern "C" int srk_usm_table_host(int K, double sigma, double* g) {
#pragma clang fp contract(off)
  SRK_REQUIRE(g, "usm_table_host: null pointer");
  SRK_REQUIRE(K >= 1 && K <= kUsmMaxK && (K & 1), "usm_table_host: K must be odd and in [1, %d] (got %d)", kUsmMaxK, K);
  if (sigma <= 0.0) sigma = 0.3 * ((K - 1) * 0.5 - 1.0) + 0.8;   // cv2.getGaussianKernel's rule for "sigma 0"
  const int c = K / 2;
  for (int i = 0; i < K; ++i) {
    const double d = (double)(i - c);
    g[i] = exp(-(d * d) / (2.0 * (sigma * sigma)));
  }
  double sum = 0.0, comp = 0.0;   // Neumaier, as srk_blur_weights_host
  for (int i = 0; i < K; ++i) {
    const double e = g[i], t = sum + e;
    comp += fabs(sum) >= fabs(e) ? (sum - t) + e : (e - t) + sum;
    sum = t;
  }
  sum += comp;
  for (int i = 0; i < K; ++i) g[i] /= sum;
  sum = comp = 0.0;               // the centre tap takes up what the rounded taps' sum lacks from 1 (srk_blur_table_host)
  for (int i = 0; i < K; ++i) {
    const double e = g[i], t = sum + e;
    comp += fabs(sum) >= fabs(e) ? (sum - t) + e : (e - t) + sum;
    sum = t;
  }
  g[c] -= (sum - 1.0) + comp;
  return SRK_OK;
}

// One plane's separable pass on the host: bytes a [H][W] -> out fp64 [H][W], through the padded copies the tile stands for.
static void usm_blur_host(const uint8_t* a, const double* g, int K, int H, int W, std::vector<uint8_t>& pad,
                          std::vector<double>& rows, double* out) {
  const int r = K / 2, PH = H + 2 * r, PW = W + 2 * r;
  pad.resize((size_t)PH * PW);
  rows.resize((size_t)PH * W);
  for (int i = 0; i < PH; ++i)
    for (int j = 0; j < PW; ++j) pad[(size_t)i * PW + j] = a[(size_t)usm_reflect(i - r, H, r) * W + usm_reflect(j - r, W, r)];
  for (int i = 0; i < PH; ++i)
    for (int j = 0; j < W; ++j) rows[(size_t)i * W + j] = usm_taps(g, pad.data() + (size_t)i * PW + j, 1, K);
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < W; ++j) out[(size_t)i * W + j] = usm_taps(g, rows.data() + (size_t)i * W + j, W, K);
}

extern "C" int srk_usm_u8_host(const uint8_t* x, uint8_t* y, const double* g, int K, double weight, double threshold, int B,
                               int C, int H, int W) {
  if (int rc = usm_check("usm_u8_host", x, y, g, K, B, C, H, W)) return rc;
  const size_t hw = (size_t)H * W;
  std::vector<uint8_t> pad, mask(hw);
  std::vector<double> rows, res(hw), soft(hw);
  for (size_t pl = 0; pl < (size_t)B * C; ++pl) {
    const uint8_t* p = x + pl * hw;
    usm_blur_host(p, g, K, H, W, pad, rows, soft.data());
    for (size_t e = 0; e < hw; ++e) usm_residual(p[e], soft[e], threshold, &res[e], &mask[e]);
    usm_blur_host(mask.data(), g, K, H, W, pad, rows, soft.data());
    for (size_t e = 0; e < hw; ++e) y[pl * hw + e] = usm_finish(p[e], res[e], soft[e], weight);
  }
  return SRK_OK;
}
