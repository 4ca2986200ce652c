// The multi-layer VGG feature loss (Real-ESRGAN's: an L1 on VGG19 maps taken before their ReLUs), one tapped layer per
// launch: the tap reads the two pre-activation maps once, adds up |a - b|, and runs what the head runs behind the tap --
// ReLU and the 2 x 2 max-pool, or the ReLU alone -- for both operands in the same pass.  The backward forms the L1 gradient
// and the pool's (k_maxpool2_bwd's rule, relu_input = 1) in one write of da.  Definition: include/srk.h; DESIGN.md 33.
// HBM-bound streaming kernels under the rules of DESIGN.md 13.6: grid_for, Vec<V>, per-block fp64 partials, one finish.
#include "srk_common.h"
#include "vgg_tap_common.h"

namespace srk {

// The blocks beyond the grid get their zero from block 0, so the finish adds whole rows whatever grids wrote them.
__device__ __forceinline__ void vgg_tap_store_partial(double acc, double scale, double* sm, double* __restrict__ rowp) {
  store_block_sum_256_d(acc * scale, sm, rowp + blockIdx.x);
  if (blockIdx.x == 0)
    for (int i = (int)gridDim.x + (int)threadIdx.x; i < kVggTapPartials; i += 256) rowp[i] = 0.0;
}

// One thread owns one 2 x 2 window of V channels.  The window grid is ceil(H/2) x ceil(W/2); the eight loads are
// unconditional, from indices clamped into the maps, and selected afterwards (k_maxpool2_bwd).
struct TapWindow {
  size_t i00, i01, i10, i11, ip;
  bool has_x1, has_y1;
};

template <int V>
__device__ __forceinline__ TapWindow tap_window(size_t e, int H, int W, int C) {
  const int OH = H / 2, OW = W / 2, WH = (H + 1) / 2, WW = (W + 1) / 2, CG = C / V;
  const int cg = (int)(e % CG);
  size_t t = e / CG;
  const int wx = (int)(t % WW);
  t /= WW;
  const int wy = (int)(t % WH);
  const size_t n = t / WH;
  const int y0 = 2 * wy, x0 = 2 * wx;   // always inside the plane
  TapWindow q;
  q.has_y1 = y0 + 1 < H;
  q.has_x1 = x0 + 1 < W;
  const int y1 = q.has_y1 ? y0 + 1 : y0, x1 = q.has_x1 ? x0 + 1 : x0;   // clamped: loads stay inside a and b
  const int py = wy < OH ? wy : OH - 1, px = wx < OW ? wx : OW - 1;     // ... and inside the pooled maps
  const size_t c0 = (size_t)cg * V;
  const size_t r0 = (n * H + y0) * W, r1 = (n * H + y1) * W;
  q.i00 = (r0 + x0) * C + c0, q.i01 = (r0 + x1) * C + c0, q.i10 = (r1 + x0) * C + c0, q.i11 = (r1 + x1) * C + c0;
  q.ip = ((n * OH + py) * OW + px) * C + c0;
  return q;
}

template <int V>
__global__ __launch_bounds__(256) void k_vgg_tap_pool_fwd(const float* __restrict__ a, const float* __restrict__ b,
                                                          float* __restrict__ ya, float* __restrict__ yb, int H, int W,
                                                          int C, size_t total, double scale, double* __restrict__ rowp) {
  typedef Vec<V> Q;
  __shared__ double sm[4];
  double acc = 0.0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const TapWindow q = tap_window<V>(e, H, W, C);
    // (every index is a multiple of V floats: C % V == 0)
    const typename Q::T a0 = Q::load(a + q.i00, 0), a1 = Q::load(a + q.i01, 0), a2 = Q::load(a + q.i10, 0),
                        a3 = Q::load(a + q.i11, 0);
    const typename Q::T b0 = Q::load(b + q.i00, 0), b1 = Q::load(b + q.i01, 0), b2 = Q::load(b + q.i10, 0),
                        b3 = Q::load(b + q.i11, 0);
    typename Q::T oa, ob;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float va[4] = {Q::at(a0, i), Q::at(a1, i), Q::at(a2, i), Q::at(a3, i)};
      const float vb[4] = {Q::at(b0, i), Q::at(b1, i), Q::at(b2, i), Q::at(b3, i)};
      float pa, pb;
      acc += vgg_tap_window_fwd(va, vb, q.has_x1, q.has_y1, &pa, &pb);
      Q::set(oa, i, pa);
      Q::set(ob, i, pb);
    }
    if (q.has_x1 && q.has_y1) {
      Q::store(ya + q.ip, 0, oa);
      Q::store(yb + q.ip, 0, ob);
    }
  }
  vgg_tap_store_partial(acc, scale, sm, rowp);
}

// RELU: ya = relu(a), yb = relu(b); LAST: the sum alone.  One thread, V consecutive floats a pass.
template <int V, bool RELU>
__global__ __launch_bounds__(256) void k_vgg_tap_elem_fwd(const float* __restrict__ a, const float* __restrict__ b,
                                                          float* __restrict__ ya, float* __restrict__ yb, size_t groups,
                                                          double scale, double* __restrict__ rowp) {
  typedef Vec<V> Q;
  __shared__ double sm[4];
  double acc = 0.0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < groups; e += (size_t)gridDim.x * 256) {
    const typename Q::T va = Q::load(a, e), vb = Q::load(b, e);
    typename Q::T oa, ob;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      acc += vgg_tap_term(Q::at(va, i), Q::at(vb, i));
      Q::set(oa, i, vgg_tap_relu(Q::at(va, i)));
      Q::set(ob, i, vgg_tap_relu(Q::at(vb, i)));
    }
    if (RELU) {
      Q::store(ya, e, oa);
      Q::store(yb, e, ob);
    }
  }
  vgg_tap_store_partial(acc, scale, sm, rowp);
}

__global__ __launch_bounds__(256) void k_vgg_tap_finish(const double* __restrict__ ws, int nparts, float* __restrict__ loss) {
  __shared__ double sm[4];
  const double tot = sum_partials_256_d(ws, nparts, sm);
  if (threadIdx.x == 0) *loss = (float)tot;
}

__device__ __forceinline__ float tap_coeff(double c, const float* __restrict__ factor) {
  return factor ? (float)(c * (double)factor[0]) : (float)c;
}

template <int V>
__global__ __launch_bounds__(256) void k_vgg_tap_pool_bwd(const float* __restrict__ a, const float* __restrict__ b,
                                                          const float* __restrict__ g, float* __restrict__ da, int H, int W,
                                                          int C, size_t total, double c, const float* __restrict__ factor) {
  typedef Vec<V> Q;
  const float cs = tap_coeff(c, factor);
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const TapWindow q = tap_window<V>(e, H, W, C);
    const typename Q::T a0 = Q::load(a + q.i00, 0), a1 = Q::load(a + q.i01, 0), a2 = Q::load(a + q.i10, 0),
                        a3 = Q::load(a + q.i11, 0);
    const typename Q::T b0 = Q::load(b + q.i00, 0), b1 = Q::load(b + q.i01, 0), b2 = Q::load(b + q.i10, 0),
                        b3 = Q::load(b + q.i11, 0);
    const typename Q::T gv = Q::load(g + q.ip, 0);
    typename Q::T o0, o1, o2, o3;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float va[4] = {Q::at(a0, i), Q::at(a1, i), Q::at(a2, i), Q::at(a3, i)};
      const float vb[4] = {Q::at(b0, i), Q::at(b1, i), Q::at(b2, i), Q::at(b3, i)};
      float d[4];
      vgg_tap_window_bwd<float>(va, vb, Q::at(gv, i), cs, q.has_x1 && q.has_y1, d);
      Q::set(o0, i, d[0]);
      Q::set(o1, i, d[1]);
      Q::set(o2, i, d[2]);
      Q::set(o3, i, d[3]);
    }
    Q::store(da + q.i00, 0, o0);
    if (q.has_x1) Q::store(da + q.i01, 0, o1);
    if (q.has_y1) {
      Q::store(da + q.i10, 0, o2);
      if (q.has_x1) Q::store(da + q.i11, 0, o3);
    }
  }
}

template <int V, bool RELU>
__global__ __launch_bounds__(256) void k_vgg_tap_elem_bwd(const float* __restrict__ a, const float* __restrict__ b,
                                                          const float* __restrict__ g, float* __restrict__ da, size_t groups,
                                                          double c, const float* __restrict__ factor) {
  typedef Vec<V> Q;
  const float cs = tap_coeff(c, factor);
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < groups; e += (size_t)gridDim.x * 256) {
    const typename Q::T va = Q::load(a, e), vb = Q::load(b, e);
    typename Q::T gv = va;   // (LAST: no gradient map is read)
    if (RELU) gv = Q::load(g, e);
    typename Q::T o;
#pragma unroll
    for (int i = 0; i < V; ++i) Q::set(o, i, vgg_tap_elem_bwd<float>(Q::at(va, i), Q::at(vb, i), Q::at(gv, i), cs, RELU));
    Q::store(da, e, o);
  }
}

struct TapPlan {
  size_t items;
  unsigned blocks;
};

// The one grid rule of both directions: windows (POOL) or elements (RELU, LAST), in groups of 4 channels on the 16-byte
// path; a block per 256 window groups (eight 16-byte loads a thread and pass), per 512 of anything else; at most
// kVggTapPartials blocks, the slots of a workspace row.
inline TapPlan tap_plan(int N, int H, int W, int C, int mode, bool vec) {
  TapPlan p;
  const size_t units = mode == SRK_VGG_TAP_POOL ? (size_t)N * ((H + 1) / 2) * ((W + 1) / 2) : (size_t)N * H * W;
  p.items = vec ? units * (C / 4) : units * C;
  p.blocks = grid_for(p.items, (mode == SRK_VGG_TAP_POOL && vec) ? 256 : 512, kVggTapPartials);
  return p;
}

inline bool tap_mode_ok(int mode) {
  return mode == SRK_VGG_TAP_POOL || mode == SRK_VGG_TAP_RELU || mode == SRK_VGG_TAP_LAST;
}

}  // namespace srk

using namespace srk;

#define SRK_TAP_DIMS(what)                                                                                   \
  SRK_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, what ": bad dims");                                          \
  SRK_REQUIRE(tap_mode_ok(mode), what ": mode %d is none of SRK_VGG_TAP_POOL / _RELU / _LAST", mode);         \
  SRK_REQUIRE(mode != SRK_VGG_TAP_POOL || (H >= 2 && W >= 2), what ": a %d x %d plane has no 2 x 2 window", H, W)

extern "C" size_t srk_vgg_tap_workspace_bytes(int rows) {
  return rows > 0 ? (size_t)rows * kVggTapPartials * sizeof(double) : 0;
}

extern "C" int srk_vgg_tap_plan(int N, int H, int W, int C, int mode, int vec, long long* items) {
  SRK_TAP_DIMS("vgg_tap_plan");
  SRK_REQUIRE(!vec || C % 4 == 0, "vgg_tap_plan: the 16-byte path needs C %% 4 == 0 (got %d)", C);
  const TapPlan p = tap_plan(N, H, W, C, mode, vec != 0);
  if (items) *items = (long long)p.items;
  return (int)p.blocks;
}

extern "C" int srk_vgg_tap_forward(const float* a, const float* b, int N, int H, int W, int C, int mode, double weight,
                                   int row, int rows, void* workspace, float* ya, float* yb, void* stream) {
  SRK_REQUIRE(a && b && workspace, "vgg_tap_forward: null pointer");
  SRK_TAP_DIMS("vgg_tap_forward");
  SRK_REQUIRE(mode == SRK_VGG_TAP_LAST || (ya && yb), "vgg_tap_forward: null pointer (the maps behind the tap)");
  SRK_REQUIRE(weight >= 0.0 && weight < (double)INFINITY, "vgg_tap_forward: weight %g is not a finite number >= 0", weight);
  SRK_REQUIRE(rows > 0 && row >= 0 && row < rows, "vgg_tap_forward: row %d of a workspace of %d rows", row, rows);
  SRK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "vgg_tap_forward: workspace is not 8-byte aligned");
  const bool last = mode == SRK_VGG_TAP_LAST;
  const bool vec = C % 4 == 0 && aligned16(a, b) && (last || aligned16(ya, yb));
  const TapPlan p = tap_plan(N, H, W, C, mode, vec);
  const double scale = weight / ((double)N * H * W * C);
  double* rowp = (double*)workspace + (size_t)row * kVggTapPartials;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(p.blocks), block(256);
  if (mode == SRK_VGG_TAP_POOL)
    hipLaunchKernelGGL(vec ? k_vgg_tap_pool_fwd<4> : k_vgg_tap_pool_fwd<1>, grid, block, 0, s, a, b, ya, yb, H, W, C, p.items,
                       scale, rowp);
  else if (mode == SRK_VGG_TAP_RELU)
    hipLaunchKernelGGL((vec ? k_vgg_tap_elem_fwd<4, true> : k_vgg_tap_elem_fwd<1, true>), grid, block, 0, s, a, b, ya, yb,
                       p.items, scale, rowp);
  else
    hipLaunchKernelGGL((vec ? k_vgg_tap_elem_fwd<4, false> : k_vgg_tap_elem_fwd<1, false>), grid, block, 0, s, a, b,
                       (float*)nullptr, (float*)nullptr, p.items, scale, rowp);
  return check_launch("vgg_tap_forward");
}

extern "C" int srk_vgg_tap_finish(const void* workspace, int rows, float* loss, void* stream) {
  SRK_REQUIRE(workspace && loss, "vgg_tap_finish: null pointer");
  SRK_REQUIRE(rows > 0 && rows <= (1 << 16), "vgg_tap_finish: %d rows", rows);
  hipLaunchKernelGGL(k_vgg_tap_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace,
                     rows * kVggTapPartials, loss);
  return check_launch("vgg_tap_finish");
}

extern "C" int srk_vgg_tap_backward(const float* a, const float* b, const float* g, int N, int H, int W, int C, int mode,
                                    double c, const float* factor, float* da, void* stream) {
  SRK_REQUIRE(a && b && da, "vgg_tap_backward: null pointer");
  SRK_TAP_DIMS("vgg_tap_backward");
  SRK_REQUIRE(mode == SRK_VGG_TAP_LAST || g, "vgg_tap_backward: null pointer (the gradient of the map behind the tap)");
  SRK_REQUIRE(c == c && c > -(double)INFINITY && c < (double)INFINITY, "vgg_tap_backward: c is not finite");
  const bool last = mode == SRK_VGG_TAP_LAST;
  const bool vec = C % 4 == 0 && aligned16(a, b, da) && (last || aligned16(g));
  const TapPlan p = tap_plan(N, H, W, C, mode, vec);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(p.blocks), block(256);
  if (mode == SRK_VGG_TAP_POOL)
    hipLaunchKernelGGL(vec ? k_vgg_tap_pool_bwd<4> : k_vgg_tap_pool_bwd<1>, grid, block, 0, s, a, b, g, da, H, W, C, p.items,
                       c, factor);
  else if (mode == SRK_VGG_TAP_RELU)
    hipLaunchKernelGGL((vec ? k_vgg_tap_elem_bwd<4, true> : k_vgg_tap_elem_bwd<1, true>), grid, block, 0, s, a, b, g, da,
                       p.items, c, factor);
  else
    hipLaunchKernelGGL((vec ? k_vgg_tap_elem_bwd<4, false> : k_vgg_tap_elem_bwd<1, false>), grid, block, 0, s, a, b,
                       (const float*)nullptr, da, p.items, c, factor);
  return check_launch("vgg_tap_backward");
}

// ---- the host twins: the same bodies over the same windows, in index order ------------------------------------------------
namespace {
struct HostWindow {
  size_t i[4], ip;
  bool has_x1, has_y1;
};
inline HostWindow host_window(size_t n, int wy, int wx, int ch, int H, int W, int C) {
  const int OH = H / 2, OW = W / 2;
  HostWindow q;
  const int y0 = 2 * wy, x0 = 2 * wx;
  q.has_y1 = y0 + 1 < H;
  q.has_x1 = x0 + 1 < W;
  const int y1 = q.has_y1 ? y0 + 1 : y0, x1 = q.has_x1 ? x0 + 1 : x0;
  const size_t r0 = (n * H + y0) * W, r1 = (n * H + y1) * W;
  q.i[0] = (r0 + x0) * C + ch, q.i[1] = (r0 + x1) * C + ch, q.i[2] = (r1 + x0) * C + ch, q.i[3] = (r1 + x1) * C + ch;
  q.ip = (q.has_x1 && q.has_y1) ? ((n * OH + wy) * OW + wx) * C + ch : 0;
  return q;
}
}  // namespace

extern "C" int srk_vgg_tap_forward_host(const float* a, const float* b, int N, int H, int W, int C, int mode, double weight,
                                        double* loss, float* ya, float* yb) {
  SRK_REQUIRE(a && b && loss, "vgg_tap_forward_host: null pointer");
  SRK_TAP_DIMS("vgg_tap_forward_host");
  SRK_REQUIRE(mode == SRK_VGG_TAP_LAST || (ya && yb), "vgg_tap_forward_host: null pointer (the maps behind the tap)");
  SRK_REQUIRE(weight >= 0.0 && weight < (double)INFINITY, "vgg_tap_forward_host: weight %g is not a finite number >= 0",
              weight);
  const size_t total = (size_t)N * H * W * C;
  double acc = 0.0;
  if (mode == SRK_VGG_TAP_POOL) {
    for (size_t n = 0; n < (size_t)N; ++n)
      for (int wy = 0; wy < (H + 1) / 2; ++wy)
        for (int wx = 0; wx < (W + 1) / 2; ++wx)
          for (int ch = 0; ch < C; ++ch) {
            const HostWindow q = host_window(n, wy, wx, ch, H, W, C);
            const float va[4] = {a[q.i[0]], a[q.i[1]], a[q.i[2]], a[q.i[3]]};
            const float vb[4] = {b[q.i[0]], b[q.i[1]], b[q.i[2]], b[q.i[3]]};
            float pa, pb;
            acc += vgg_tap_window_fwd(va, vb, q.has_x1, q.has_y1, &pa, &pb);
            if (q.has_x1 && q.has_y1) ya[q.ip] = pa, yb[q.ip] = pb;
          }
  } else {
    for (size_t e = 0; e < total; ++e) {
      acc += vgg_tap_term(a[e], b[e]);
      if (mode == SRK_VGG_TAP_RELU) ya[e] = vgg_tap_relu(a[e]), yb[e] = vgg_tap_relu(b[e]);
    }
  }
  *loss = acc * (weight / (double)total);
  return SRK_OK;
}

extern "C" int srk_vgg_tap_backward_host(const float* a, const float* b, const float* g, int N, int H, int W, int C, int mode,
                                         double c, float* da) {
  SRK_REQUIRE(a && b && da, "vgg_tap_backward_host: null pointer");
  SRK_TAP_DIMS("vgg_tap_backward_host");
  SRK_REQUIRE(mode == SRK_VGG_TAP_LAST || g, "vgg_tap_backward_host: null pointer (the gradient of the map behind the tap)");
  if (mode == SRK_VGG_TAP_POOL) {
    for (size_t n = 0; n < (size_t)N; ++n)
      for (int wy = 0; wy < (H + 1) / 2; ++wy)
        for (int wx = 0; wx < (W + 1) / 2; ++wx)
          for (int ch = 0; ch < C; ++ch) {
            const HostWindow q = host_window(n, wy, wx, ch, H, W, C);
            const float va[4] = {a[q.i[0]], a[q.i[1]], a[q.i[2]], a[q.i[3]]};
            const float vb[4] = {b[q.i[0]], b[q.i[1]], b[q.i[2]], b[q.i[3]]};
            const bool whole = q.has_x1 && q.has_y1;
            float d[4];
            vgg_tap_window_bwd<double>(va, vb, whole ? g[q.ip] : 0.f, c, whole, d);
            da[q.i[0]] = d[0];
            if (q.has_x1) da[q.i[1]] = d[1];
            if (q.has_y1) {
              da[q.i[2]] = d[2];
              if (q.has_x1) da[q.i[3]] = d[3];
            }
          }
  } else {
    const size_t total = (size_t)N * H * W * C;
    const bool relu = mode == SRK_VGG_TAP_RELU;
    for (size_t e = 0; e < total; ++e) da[e] = vgg_tap_elem_bwd<double>(a[e], b[e], relu ? g[e] : 0.f, c, relu);
  }
  return SRK_OK;
}
