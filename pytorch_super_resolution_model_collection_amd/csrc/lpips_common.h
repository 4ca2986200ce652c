// What the LPIPS layer kernels (lpips.hip: k_lpips<V, R, BWD>) and their host twin (srk_lpips_layer_host) share:
// the planner and the arithmetic of one pixel, one element per call so that the lanes sharing a pixel spread the
// channels over themselves and the host loops over them.  Definition: include/srk.h and DESIGN.md 27.
//   a = ||f0||_2 + eps, b = ||f1||_2 + eps (over the pixel's channels), q[c] = f0[c] / a - f1[c] / b
//   d = sum_c w[c] q[c]^2
//   dd/df0[k] = 2 w[k] q[k] / a - f0[k] / (a^2 r) * sum_c 2 w[c] q[c] f0[c],  r = ||f0||_2; the second term is 0 where r == 0
// The normalised values are subtracted (never the expanded quadratic form), so f0 == f1 gives q == 0, d == 0 and a zero
// gradient exactly.  All of it is double on the fp32 inputs; 1 / a is taken once a pixel and multiplied in.
#ifndef SRK_LPIPS_COMMON_H_
#define SRK_LPIPS_COMMON_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace srk {

constexpr double kLpipsEps = 1e-10;
constexpr int kLpipsMaxHeld = 8;        // channel groups a lane keeps in registers, at most; beyond that a pixel is re-read
constexpr int kLpipsPassesPerBlock = 4; // pixel passes of a block, at least, before another block is opened
constexpr int kLpipsMaxBlocks = 1024;   // partial blocks per sample, at most: one block adds them up again

struct LpipsPlan {
  int V;        // floats per access (4 or 1)
  int G;        // channel groups of V floats per pixel
  int L;        // lanes that share a pixel: a power of two, at most 64
  int R;        // groups per lane held in registers (1, 2, 4 or 8), or 0: the pixel is read twice
  int blocks;   // blocks (= partial sums) per sample
};

// vec: C % 4 == 0 and every pointer on a 16-byte boundary
__host__ __device__ __forceinline__ LpipsPlan lpips_plan(int64_t hw, int C, bool vec) {
  LpipsPlan p;
  p.V = vec ? 4 : 1;
  p.G = C / p.V;
  p.L = 1;
  while (p.L < 64 && p.L < p.G) p.L *= 2;
  const int per = (p.G + p.L - 1) / p.L;
  p.R = per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= kLpipsMaxHeld ? 8 : 0;
  const int64_t pixels_per_pass = 256 / p.L;
  const int64_t b = (hw + pixels_per_pass * kLpipsPassesPerBlock - 1) / (pixels_per_pass * kLpipsPassesPerBlock);
  p.blocks = (int)(b < 1 ? 1 : (b > kLpipsMaxBlocks ? kLpipsMaxBlocks : b));
  return p;
}

// one more channel of a pixel's sum of squares
__host__ __device__ __forceinline__ double lpips_ss(float f, double ss) { return fma((double)f, (double)f, ss); }

// one more channel of d = sum_c w q^2, and of S = sum_c 2 w q f0
__host__ __device__ __forceinline__ double lpips_term(float w, double q, double d) { return fma((double)w * q, q, d); }
__host__ __device__ __forceinline__ double lpips_pull_term(float w, double q, float f0, double S) {
  return fma(2.0 * (double)w * q, (double)f0, S);
}

// 1 / (||f|| + eps) from the pixel's sum of squares
__host__ __device__ __forceinline__ double lpips_inv_norm(double ss) { return 1.0 / (sqrt(ss) + kLpipsEps); }

// q = f0 / a - f1 / b: two rounded products, then the difference.  Contracted into fma(f0, 1 / a, -(f1 / b)) the first
// product would stay unrounded, and equal maps would leave the rounding error of the second instead of an exact zero.
__host__ __device__ __forceinline__ double lpips_q(float f0, float f1, double ia, double ib) {
#pragma clang fp contract(off)
  const double x = (double)f0 * ia, y = (double)f1 * ib;
  return x - y;
}

// the factor of f0[k] in the gradient's second term: S / (a^2 r), S = sum_c 2 w q f0; 0 where r == 0 (its limit)
__host__ __device__ __forceinline__ double lpips_pull(double ss0, double ia, double S) {
  return ss0 > 0.0 ? ia * ia * S / sqrt(ss0) : 0.0;
}

// dd/df0[k] times the upstream factor `up`
__host__ __device__ __forceinline__ double lpips_grad(float f0, float w, double q, double ia, double pull, double up) {
  return up * (2.0 * (double)w * q * ia - (double)f0 * pull);
}

}  // namespace srk
#endif  // SRK_LPIPS_COMMON_H_
