// What the device NIQE features (niqe.hip: k_niqe_scale) and their host twin (srk_niqe_features_host) share: the luma
// rule, the 7-tap window, the 2:1 shrink, the per-map sums and the AGGD fit.  include/srk.h has the definition,
// DESIGN.md 34 the arithmetic.
#ifndef SRK_NIQE_COMMON_H_
#define SRK_NIQE_COMMON_H_
#include <math.h>

#include "color_common.h"

namespace srk {

constexpr int kNiqeTaps = 7, kNiqeHalo = kNiqeTaps - 1, kNiqeR = kNiqeTaps / 2;
constexpr int kNiqeShrinkTaps = 8;
constexpr int kNiqeTable = SRK_NIQE_TABLE;
constexpr int kNiqeMaps = 5, kNiqeSums = 6;   // per map: c_neg, q_neg, c_pos, q_pos, a, q
constexpr int kNiqeMinBlock = 8, kNiqeMaxBlock = 96;

// g[i] = exp(-(i - 3)^2 / (2 (7/6)^2)) / sum, to 17 significant digits (the doubles numpy's exp and division give).
struct NiqeWindow {
  double g[kNiqeTaps];
};
constexpr NiqeWindow make_niqe_window() {
  return {{0.012560200468474614, 0.07882796468173002, 0.2372960771171706, 0.34263151546524945, 0.2372960771171706,
           0.07882796468173002, 0.012560200468474614}};
}
static constexpr NiqeWindow kNiqeWinHost = make_niqe_window();
__constant__ const NiqeWindow kNiqeWinDev = make_niqe_window();

// MATLAB's antialiased bicubic at scale 1/2: the cubic kernel (a = -0.5) widened by 2 and sampled at the eight half-odd
// distances (2i - 3 + k) - (2i + 0.5) of output i, times 1/2; the eight sum to 1 and are exact in binary.
__host__ __device__ __forceinline__ double niqe_shrink_weight(int k) {
  const int w[kNiqeShrinkTaps] = {-3, -9, 29, 111, 111, 29, -9, -3};
  return w[k] * (1.0 / 256.0);
}
// symmetric reflection with the edge sample repeated: -1 -> 0, -2 -> 1, n -> n - 1 (|overshoot| <= n)
__host__ __device__ __forceinline__ int niqe_reflect(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

// BT.601 studio-range luma of three bytes, rounded to nearest-even.  Contraction is off so that the host, the device
// and numpy round the very same five operations.
__host__ __device__ __forceinline__ double niqe_luma(unsigned r, unsigned g, unsigned b) {
#pragma clang fp contract(off)
  const double s = 65.481 * (double)r + 128.553 * (double)g + 24.966 * (double)b;
  return rint(16.0 + s / 255.0);
}
// The picture as the caller holds it: [C][H][W] through element strides, fp32 (quantised by quant_u8 on the way) or
// bytes; origin = the crop's first pixel in elements.  (y, x) are coordinates inside the crop.
struct NiqeSrc {
  const void* img;
  int is_u8, C;
  int64_t sc, sh, sw, origin;
};
__host__ __device__ __forceinline__ double niqe_src_luma(const NiqeSrc& s, int y, int x) {
  const int64_t o = s.origin + (int64_t)y * s.sh + (int64_t)x * s.sw;
  unsigned v[3] = {0u, 0u, 0u};
  for (int ch = 0; ch < s.C; ++ch)
    v[ch] = s.is_u8 ? (unsigned)static_cast<const uint8_t*>(s.img)[o + ch * s.sc]
                    : quant_u8(static_cast<const float*>(s.img)[o + ch * s.sc]);
  return s.C == 3 ? niqe_luma(v[0], v[1], v[2]) : (double)v[0];
}

__host__ __device__ __forceinline__ double niqe_mscn(double p, double mu, double ex2) {
#pragma clang fp contract(off)
  return (p - mu) / (sqrt(fabs(ex2 - mu * mu)) + 1.0);
}
__host__ __device__ __forceinline__ double niqe_sigma(double mu, double ex2) {
#pragma clang fp contract(off)
  return sqrt(fabs(ex2 - mu * mu));
}

// one value of one map into that map's six sums
__host__ __device__ __forceinline__ void niqe_accumulate(double* s, double m) {
#pragma clang fp contract(off)
  const double m2 = m * m;
  if (m < 0.0) s[0] += 1.0, s[1] += m2;
  if (m > 0.0) s[2] += 1.0, s[3] += m2;
  s[4] += fabs(m);
  s[5] += m2;
}

// argmin_j (r_gam[j] - rn)^2 with numpy's first-index tie rule, on the increasing table: the first j with r_gam[j] >= rn
// by bisection, then the exact squared differences of j - 1 and j.  rn beyond either end clamps; a NaN rn gives 0.
__host__ __device__ __forceinline__ int niqe_table_index(const double* __restrict__ r_gam, double rn) {
#pragma clang fp contract(off)
  int lo = 0, hi = kNiqeTable;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (r_gam[mid] < rn) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return 0;
  if (lo == kNiqeTable) return kNiqeTable - 1;
  const double d0 = (r_gam[lo - 1] - rn) * (r_gam[lo - 1] - rn), d1 = (r_gam[lo] - rn) * (r_gam[lo] - rn);
  return d1 < d0 ? lo : lo - 1;
}
__host__ __device__ __forceinline__ double niqe_gam(int j) {
#pragma clang fp contract(off)
  const double step = (0.2 + 0.001) - 0.2;   // numpy's arange: start + j * ((start + step) - start)
  return 0.2 + (double)j * step;
}

// The AGGD fit of one map from its six sums over M values: map 0 writes two features, a product map four.
// tables: [3][kNiqeTable] = r_gam, sqrt(Gamma(1/g) / Gamma(3/g)), Gamma(2/g) / Gamma(1/g).
__host__ __device__ __forceinline__ void niqe_fit(const double* s, double M, const double* __restrict__ tables, int map,
                                                   double* __restrict__ out) {
#pragma clang fp contract(off)
  const int nout = map == 0 ? 2 : 4;
  if (s[0] == 0.0 || s[2] == 0.0 || s[5] == 0.0) {
    for (int i = 0; i < nout; ++i) out[i] = NAN;
    return;
  }
  const double ls = sqrt(s[1] / s[0]), rs = sqrt(s[3] / s[2]), gh = ls / rs;
  const double am = s[4] / M;
  const double rhat = (am * am) / (s[5] / M);
  const double g2 = gh * gh;
  const double rn = rhat * (g2 * gh + 1.0) * (gh + 1.0) / ((g2 + 1.0) * (g2 + 1.0));
  const int j = niqe_table_index(tables, rn);
  const double alpha = niqe_gam(j), t1 = tables[kNiqeTable + j], t2 = tables[2 * kNiqeTable + j];
  const double bl = ls * t1, br = rs * t1;
  out[0] = alpha;
  if (map == 0) {
    out[1] = (bl + br) / 2.0;
  } else {
    out[1] = (br - bl) * t2;
    out[2] = bl;
    out[3] = br;
  }
}
__host__ __device__ __forceinline__ int niqe_feature_offset(int map) { return map == 0 ? 0 : 2 + 4 * (map - 1); }

// the other factor of product map k at (r, c) of a b x b block: roll(B, shift_k)[r][c] = B[(r - dr) mod b][(c - dc) mod b]
__host__ __device__ __forceinline__ void niqe_roll_source(int k, int r, int c, int b, int& rr, int& cc) {
  const int dr = k == 1 ? 0 : 1, dc = k == 2 ? 0 : (k == 4 ? -1 : 1);
  rr = r - dr, cc = c - dc;
  if (rr < 0) rr += b;
  if (cc < 0) cc += b;
  if (cc >= b) cc -= b;
}

}  // namespace srk
#endif  // SRK_NIQE_COMMON_H_
