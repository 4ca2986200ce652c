// What the channel-attention kernels (ca.hip: k_ca_gate_apply / k_ca_bwd_apply) and their host twin
// (srk_channel_attention_host) share: the supported range, the planner, and the squeeze-excite MLP forward and backward,
// one output element per call so that a block spreads them over its threads and the host loops over them.  DESIGN.md 25.
//   h = relu(W1 m + b1),  s = sigmoid(W2 h + b2)            W1 [Cr][C], W2 [C][Cr], row-major (a 1x1 conv's [out][in])
//   da = ds * s * (1 - s),  dh = (W2^T da) where h > 0,  dm = W1^T dh
// All of it is double: 2 * C * Cr products a sample, nothing next to the image-sized passes around it.
#ifndef SRK_CA_COMMON_H_
#define SRK_CA_COMMON_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srk {

constexpr int kCaMaxC = 256;    // SRK_CA_MAX_C: a block finishes one column per thread
constexpr int kCaMaxCr = 64;    // SRK_CA_MAX_CR
constexpr int kCaSplitRows = 128;   // pixels of a sample per partial block, at least
constexpr int kCaMaxSplits = 64;    // partial blocks per sample, at most: every block of the apply pass adds them up again

// Partial blocks per sample for the two column sums over HW.
__host__ __device__ __forceinline__ int ca_splits(int64_t hw) {
  const int64_t s = (hw + kCaSplitRows - 1) / kCaSplitRows;
  return (int)(s < 1 ? 1 : (s > kCaMaxSplits ? kCaMaxSplits : s));
}
// Pixels per block of the apply passes: the [splits][C] doubles a block re-adds stay under a twelfth of what it streams.
__host__ __device__ __forceinline__ int64_t ca_apply_rows(int splits) {
  return splits * 8 > kCaSplitRows ? splits * 8 : kCaSplitRows;
}

// The loops below are short dependent fp64 chains fed by loads that do not depend on the chain: unrolled, the loads of
// eight steps are in flight together instead of one memory latency per step (the order of the additions is unchanged).
#define SRK_CA_UNROLL _Pragma("unroll 8")

// relu that keeps a NaN (torch.relu does): a NaN pixel poisons its whole sample, and only that
__host__ __device__ __forceinline__ double ca_relu(double v) { return v < 0.0 ? 0.0 : v; }

// h[j] from the pooled means m[0..C)
template <typename M>
__host__ __device__ __forceinline__ double ca_hidden(int j, const M* m, const float* w1, const float* b1, int C) {
  double a = b1[j];
  SRK_CA_UNROLL
  for (int c = 0; c < C; ++c) a = fma((double)w1[(size_t)j * C + c], (double)m[c], a);
  return ca_relu(a);
}

// s[c] from the hidden h[0..Cr)
template <typename H>
__host__ __device__ __forceinline__ double ca_gate(int c, const H* h, const float* w2, const float* b2, int Cr) {
  double a = b2[c];
  SRK_CA_UNROLL
  for (int j = 0; j < Cr; ++j) a = fma((double)w2[(size_t)c * Cr + j], (double)h[j], a);
  return 1.0 / (1.0 + exp(-a));
}

// da[c]: the gradient at the sigmoid's argument from ds[c] = sum_hw g * t
__host__ __device__ __forceinline__ double ca_dgate(double ds, double s) { return ds * s * (1.0 - s); }

// dh[j]: zero (not 0 * x) where the hidden unit is off
template <typename H>
__host__ __device__ __forceinline__ double ca_dhidden(int j, const double* da, const float* w2, const H* h, int C, int Cr) {
  if (!((double)h[j] > 0.0)) return 0.0;
  double a = 0.0;
  SRK_CA_UNROLL
  for (int c = 0; c < C; ++c) a = fma((double)w2[(size_t)c * Cr + j], da[c], a);
  return a;
}

// dm[c], the gradient at the pooled mean (the caller divides by HW)
__host__ __device__ __forceinline__ double ca_dmean(int c, const double* dh, const float* w1, int C, int Cr) {
  double a = 0.0;
  SRK_CA_UNROLL
  for (int j = 0; j < Cr; ++j) a = fma((double)w1[(size_t)j * C + c], dh[j], a);
  return a;
}

}  // namespace srk
#endif  // SRK_CA_COMMON_H_
