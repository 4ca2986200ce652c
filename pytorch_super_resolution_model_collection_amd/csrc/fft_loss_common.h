// What the frequency-domain loss kernels (fft_loss.hip) and their host twin (srk_fft_loss_host) share: the walk through
// the twiddle table, the complex multiply-adds of the four passes, the per-bin term and the sign.  The table itself is
// DATA from one host function (srk_dft_table_host): neither side evaluates cos / sin.  DESIGN.md 26.
#ifndef SRK_FFT_LOSS_COMMON_H_
#define SRK_FFT_LOSS_COMMON_H_
#include "srk_common.h"

namespace srk {

// One entry of a table of n: (cos, sin)(2 pi k / n).
struct FftTw {
  double c, s;
};

// Index of the next twiddle along a walk: ((u * y) mod n) -> ((u * (y + 1)) mod n) is idx + u, u < n, without a division.
__host__ __device__ __forceinline__ int fft_tw_next(int idx, int step, int n) {
  idx += step;
  return idx >= n ? idx - n : idx;
}

// acc += a * exp(-i theta), a real (the row pass on the difference image).
__host__ __device__ __forceinline__ void fft_fwd_real(double a, FftTw w, double& re, double& im) {
  re = fma(a, w.c, re);
  im = fma(-a, w.s, im);
}
// acc += (ar + i ai) * exp(-i theta) (the column pass).
__host__ __device__ __forceinline__ void fft_fwd_cplx(double ar, double ai, FftTw w, double& re, double& im) {
  re = fma(ar, w.c, re);
  re = fma(ai, w.s, re);
  im = fma(ai, w.c, im);
  im = fma(-ar, w.s, im);
}
// acc += (gr + i gi) * exp(+i theta) (the adjoint column pass).
__host__ __device__ __forceinline__ void fft_adj_cplx(double gr, double gi, FftTw w, double& re, double& im) {
  re = fma(gr, w.c, re);
  re = fma(-gi, w.s, re);
  im = fma(gr, w.s, im);
  im = fma(gi, w.c, im);
}
// acc += Re((sr + i si) * exp(+i theta)) (the adjoint row pass: the gradient is real).
__host__ __device__ __forceinline__ void fft_adj_real(double sr, double si, FftTw w, double& re) {
  re = fma(sr, w.c, re);
  re = fma(-si, w.s, re);
}

// |Re F| + |Im F|: what a bin adds to the loss before the 1 / (2 M).
__host__ __device__ __forceinline__ double fft_bin_term(double re, double im) { return fabs(re) + fabs(im); }

// sign with sign(0) = 0 (either zero); a NaN stays a NaN, so that it reaches the whole plane's gradient.
__host__ __device__ __forceinline__ double fft_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : (v == 0.0 ? 0.0 : v)); }

// The sign as the kernels keep it in memory between the two column passes: the upper 16 bits of the double it stands
// for (1.0 = 0x3FF0..., -1.0 = 0xBFF0..., 0.0 = 0, a quiet NaN = 0x7FF8...; the other 48 bits of all four are zero), so
// that reading it back is one shift, not a conversion and a select per value.
__host__ __device__ __forceinline__ unsigned short fft_sign_code(double v) {
  return v > 0.0 ? (unsigned short)0x3FF0 : (v < 0.0 ? (unsigned short)0xBFF0 : (v == 0.0 ? (unsigned short)0 : (unsigned short)0x7FF8));
}
__host__ __device__ __forceinline__ double fft_sign_decode(unsigned short c) {
  const unsigned long long bits = (unsigned long long)c << 48;
  double d;
  __builtin_memcpy(&d, &bits, sizeof(d));
  return d;
}

// Columns of the Hermitian half of a real plane's spectrum: v = 0 .. W / 2.  Column v stands for itself and for W - v;
// the two edge columns (0 and, for an even W, W / 2) are their own mirrors and count once.
__host__ __device__ __forceinline__ int fft_half_cols(int W) { return W / 2 + 1; }
__host__ __device__ __forceinline__ bool fft_col_is_edge(int v, int W) { return v == 0 || 2 * v == W; }

}  // namespace srk
#endif  // SRK_FFT_LOSS_COMMON_H_
