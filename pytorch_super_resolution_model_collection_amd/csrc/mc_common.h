// Per-pixel definitions of the flow warp and the flow-smoothness term (include/srk_mc.h), shared by the
// kernels of mc.hip (T = float, sums in double) and their host twins (T = double).  Pixel coordinates, no normalisation.
#pragma once
#include <math.h>
#include <stdint.h>

namespace srk {

// The four corners and the weights of one sample at (x + fx, y + fy), clamped to the plane.  mx / my: 1 where the
// UNCLAMPED coordinate lies strictly inside (0, W - 1) / (0, H - 1), else 0 -- the factor of the flow gradient.
// A NaN flow samples pixel 0 with gradient 0: every index stays inside the plane whatever the flow holds.
template <typename T>
struct McTap {
  int x0, x1, y0, y1;
  T wx, wy, mx, my;
};

template <typename T>
__host__ __device__ inline void mc_axis(T f, int i, int n, int& i0, int& i1, T& w, T& m) {
  const T hi = (T)(n - 1);
  T s = (T)i + f;
  m = (s > (T)0 && s < hi) ? (T)1 : (T)0;
  s = !(s > (T)0) ? (T)0 : (s > hi ? hi : s);
  i0 = (int)s;                      // s >= 0: truncation is floor
  i1 = i0 + 1 < n ? i0 + 1 : n - 1;
  w = s - (T)i0;
}

template <typename T>
__host__ __device__ inline McTap<T> mc_tap(T fx, T fy, int x, int y, int H, int W) {
  McTap<T> t;
  mc_axis<T>(fx, x, W, t.x0, t.x1, t.wx, t.mx);
  mc_axis<T>(fy, y, H, t.y0, t.y1, t.wy, t.my);
  return t;
}

// The bilinear value of one plane (element strides sh, sw) at tap t, and its derivatives by the two flow components:
// d/dfx = ((v01 - v00)(1 - wy) + (v11 - v10) wy) mx, symmetric in y: on an integer coordinate the right-hand cell's slope.
template <typename T>
__host__ __device__ inline T mc_sample(const float* plane, int64_t sh, int64_t sw, const McTap<T>& t, T* dvx, T* dvy) {
  const T v00 = (T)plane[t.y0 * sh + t.x0 * sw], v01 = (T)plane[t.y0 * sh + t.x1 * sw];
  const T v10 = (T)plane[t.y1 * sh + t.x0 * sw], v11 = (T)plane[t.y1 * sh + t.x1 * sw];
  const T top = v00 + (v01 - v00) * t.wx, bot = v10 + (v11 - v10) * t.wx;
  if (dvx) *dvx = ((v01 - v00) * ((T)1 - t.wy) + (v11 - v10) * t.wy) * t.mx;
  if (dvy) *dvy = ((v10 - v00) * ((T)1 - t.wx) + (v11 - v01) * t.wx) * t.my;
  return top + (bot - top) * t.wy;
}

// Flow smoothness at pixel (y, x) of one flow [2][H][W] (element strides sc, sh, sw): the forward differences of both
// components (0 at the last column / row) and h = sqrt(eps + their squares).  d[0..3] = dx_u, dy_u, dx_v, dy_v.
__host__ __device__ inline double huber_at(const float* f, int64_t sc, int64_t sh, int64_t sw, int y, int x, int H, int W,
                                           double eps, double* d) {
  const float* p = f + y * sh + x * sw;
  const double u = p[0], v = p[sc];
  d[0] = x + 1 < W ? (double)p[sw] - u : 0.0;
  d[1] = y + 1 < H ? (double)p[sh] - u : 0.0;
  d[2] = x + 1 < W ? (double)p[sc + sw] - v : 0.0;
  d[3] = y + 1 < H ? (double)p[sc + sh] - v : 0.0;
  return sqrt(eps + d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
}

// d(sum of h) / d(u, v at (y, x)): a gather over p, p - ex, p - ey.  Returns h(p) through *h.
__host__ __device__ inline void huber_grad_at(const float* f, int64_t sc, int64_t sh, int64_t sw, int y, int x, int H, int W,
                                              double eps, double* h, double* gu, double* gv) {
  double d[4], e[4];
  *h = huber_at(f, sc, sh, sw, y, x, H, W, eps, d);
  double a = -(d[0] + d[1]) / *h, b = -(d[2] + d[3]) / *h;
  if (x > 0) {
    const double hl = huber_at(f, sc, sh, sw, y, x - 1, H, W, eps, e);
    a += e[0] / hl;
    b += e[2] / hl;
  }
  if (y > 0) {
    const double hu = huber_at(f, sc, sh, sw, y - 1, x, H, W, eps, e);
    a += e[1] / hu;
    b += e[3] / hu;
  }
  *gu = a;
  *gv = b;
}

}  // namespace srk
