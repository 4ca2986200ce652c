// Bilinear x2 upsampling of an NHWC map with a fused skip addition, and its adjoint.  Definition: include/srk.h and
// DESIGN.md 31; index and weight functions: bilinear_common.h, shared with the host twin below.
//
//   k_bilinear2x_fwd   y = up2(x + add): a thread an output pixel and V channels; four reads of x (and of add), one store.
//   k_bilinear2x_bwd   dx = up2^T(dy) in gather form: a thread an input pixel and V channels; it adds the at most 4 x 4
//                      outputs that read the pixel, rows then columns in index order.  Every dx element is written once;
//                      no atomics.  The result is the gradient of x and of add alike.
// V = 4 (16-byte accesses along C) where C % 4 == 0 and the pointers allow, else V = 1.  fp32 arithmetic in torch's order.
#include "bilinear_common.h"
#include "srk_common.h"

namespace srk {

constexpr size_t kBlMaxBlocks = 8192;

template <int V>
__global__ __launch_bounds__(256) void k_bilinear2x_fwd(const float* __restrict__ x, const float* __restrict__ add,
                                                        float* __restrict__ y, int H, int W, int CV, size_t items) {
  typedef typename Vec<V>::T T;
  const int OH = 2 * H, OW = 2 * W;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
    const int cv = (int)(i % CV);
    size_t p = i / CV;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const size_t n = p / OH;
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    bilinear2x_src<float>(oy, H, &y0, &y1, &wy0, &wy1);
    bilinear2x_src<float>(ox, W, &x0, &x1, &wx0, &wx1);
    const size_t r0 = (n * H + y0) * W, r1 = (n * H + y1) * W;
    const size_t i00 = (r0 + x0) * CV + cv, i01 = (r0 + x1) * CV + cv, i10 = (r1 + x0) * CV + cv, i11 = (r1 + x1) * CV + cv;
    T a = Vec<V>::load(x, i00), b = Vec<V>::load(x, i01), c = Vec<V>::load(x, i10), d = Vec<V>::load(x, i11);
    if (add) {
      const T a2 = Vec<V>::load(add, i00), b2 = Vec<V>::load(add, i01), c2 = Vec<V>::load(add, i10), d2 = Vec<V>::load(add, i11);
      a = a + a2, b = b + b2, c = c + c2, d = d + d2;
    }
    T o;
#pragma unroll
    for (int e = 0; e < V; ++e)
      Vec<V>::set(o, e, bilinear2x_mix<float>(Vec<V>::at(a, e), Vec<V>::at(b, e), Vec<V>::at(c, e), Vec<V>::at(d, e), wy0,
                                              wy1, wx0, wx1));
    Vec<V>::store(y, i, o);
  }
}

template <int V>
__global__ __launch_bounds__(256) void k_bilinear2x_bwd(const float* __restrict__ dy, float* __restrict__ dx, int H, int W,
                                                        int CV, size_t items) {
  typedef typename Vec<V>::T T;
  const int OH = 2 * H, OW = 2 * W;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
    const int cv = (int)(i % CV);
    size_t p = i / CV;
    const int ix = (int)(p % W);
    p /= W;
    const int iy = (int)(p % H);
    const size_t n = p / H;
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    for (int oy = 2 * iy - 1; oy <= 2 * iy + 2; ++oy) {
      const float wy = bilinear2x_adj<float>(oy, iy, H);       // 0 outside [0, 2 H): nothing is read there
      if (wy == 0.f) continue;
      for (int ox = 2 * ix - 1; ox <= 2 * ix + 2; ++ox) {
        const float wx = bilinear2x_adj<float>(ox, ix, W);
        if (wx == 0.f) continue;
        const T g = Vec<V>::load(dy, ((n * OH + oy) * OW + ox) * CV + cv);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += (wy * wx) * Vec<V>::at(g, e);
      }
    }
    T o;
#pragma unroll
    for (int e = 0; e < V; ++e) Vec<V>::set(o, e, acc[e]);
    Vec<V>::store(dx, i, o);
  }
}

static int bl_check(const char* who, int N, int H, int W, int C) {
  SRK_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 1, "%s: N = %d, H = %d, W = %d, C = %d", who, N, H, W, C);
  SRK_REQUIRE(H < (1 << 30) && W < (1 << 30), "%s: H = %d, W = %d", who, H, W);
  return SRK_OK;
}

}  // namespace srk

using namespace srk;

extern "C" int srk_upsample_bilinear2x_forward(const float* x, const float* add, float* y, int N, int H, int W, int C,
                                               void* stream) {
  const char* who = "upsample_bilinear2x_forward";
  SRK_REQUIRE(x && y, "%s: null pointer", who);
  const int rc = bl_check(who, N, H, W, C);
  if (rc != SRK_OK) return rc;
  const size_t pixels = (size_t)N * (2 * (size_t)H) * (2 * (size_t)W);
  hipStream_t s = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(x, add, y)) {
    const size_t items = pixels * (C / 4);
    hipLaunchKernelGGL(k_bilinear2x_fwd<4>, dim3(grid_for(items, 256, kBlMaxBlocks)), dim3(256), 0, s, x, add, y, H, W, C / 4,
                       items);
  } else {
    const size_t items = pixels * C;
    hipLaunchKernelGGL(k_bilinear2x_fwd<1>, dim3(grid_for(items, 256, kBlMaxBlocks)), dim3(256), 0, s, x, add, y, H, W, C,
                       items);
  }
  return check_launch(who);
}

extern "C" int srk_upsample_bilinear2x_backward(const float* dy, float* dx, int N, int H, int W, int C, void* stream) {
  const char* who = "upsample_bilinear2x_backward";
  SRK_REQUIRE(dy && dx, "%s: null pointer", who);
  const int rc = bl_check(who, N, H, W, C);
  if (rc != SRK_OK) return rc;
  const size_t pixels = (size_t)N * H * W;
  hipStream_t s = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(dy, dx)) {
    const size_t items = pixels * (C / 4);
    hipLaunchKernelGGL(k_bilinear2x_bwd<4>, dim3(grid_for(items, 256, kBlMaxBlocks)), dim3(256), 0, s, dy, dx, H, W, C / 4,
                       items);
  } else {
    const size_t items = pixels * C;
    hipLaunchKernelGGL(k_bilinear2x_bwd<1>, dim3(grid_for(items, 256, kBlMaxBlocks)), dim3(256), 0, s, dy, dx, H, W, C, items);
  }
  return check_launch(who);
}

// x, add, dy on the host, [N][H][W][C] / [N][2H][2W][C]; y and dx in double.  y == NULL or dy / dx == NULL skips that half.
extern "C" int srk_upsample_bilinear2x_host(const float* x, const float* add, const float* dy, int N, int H, int W, int C,
                                            double* y, double* dx) {
  const char* who = "upsample_bilinear2x_host";
  SRK_REQUIRE((y == nullptr) == (x == nullptr), "%s: x and y come together", who);
  SRK_REQUIRE((dy == nullptr) == (dx == nullptr), "%s: dy and dx come together", who);
  SRK_REQUIRE(y || dx, "%s: nothing to compute", who);
  SRK_REQUIRE(!add || x, "%s: add without x", who);
  const int rc = bl_check(who, N, H, W, C);
  if (rc != SRK_OK) return rc;
  const int OH = 2 * H, OW = 2 * W;
  if (y) {
    for (size_t n = 0; n < (size_t)N; ++n)
      for (int oy = 0; oy < OH; ++oy)
        for (int ox = 0; ox < OW; ++ox) {
          int y0, y1, x0, x1;
          double wy0, wy1, wx0, wx1;
          bilinear2x_src<double>(oy, H, &y0, &y1, &wy0, &wy1);
          bilinear2x_src<double>(ox, W, &x0, &x1, &wx0, &wx1);
          for (int c = 0; c < C; ++c) {
            auto at = [&](int yy, int xx) {
              const size_t i = (((n * H + yy) * W) + xx) * C + c;
              return (double)x[i] + (add ? (double)add[i] : 0.0);
            };
            y[((n * OH + oy) * OW + ox) * C + c] =
                bilinear2x_mix<double>(at(y0, x0), at(y0, x1), at(y1, x0), at(y1, x1), wy0, wy1, wx0, wx1);
          }
        }
  }
  if (dx) {
    for (size_t n = 0; n < (size_t)N; ++n)
      for (int iy = 0; iy < H; ++iy)
        for (int ix = 0; ix < W; ++ix)
          for (int c = 0; c < C; ++c) {
            double acc = 0.0;
            for (int oy = 2 * iy - 1; oy <= 2 * iy + 2; ++oy) {
              const double wy = bilinear2x_adj<double>(oy, iy, H);
              if (wy == 0.0) continue;
              for (int ox = 2 * ix - 1; ox <= 2 * ix + 2; ++ox) {
                const double wx = bilinear2x_adj<double>(ox, ix, W);
                if (wx == 0.0) continue;
                acc += (wy * wx) * (double)dy[((n * OH + oy) * OW + ox) * C + c];
              }
            }
            dx[((n * H + iy) * W + ix) * C + c] = acc;
          }
  }
  return SRK_OK;
}
