// What the channel-slice convolution kernels (dense.hip) and their host twin (srk_dense_conv_host) share: the supported
// range, the slice addressing and the planner.  DESIGN.md 28 (and 30: the _ex entry points share all of it).
//
// A "slice" is `C` channels of a wider NHWC buffer: a pointer to the slice's first channel of pixel 0 and the buffer's
// pixel stride `ld` in floats (ld >= C).  Pixel p = (n * H + h) * W + w of a slice starts at ptr + p * ld.  The input
// channels of the convolution are [A | B] in the order torch.cat((A, B), 1) gives them: channel c < CA is A's channel c,
// channel c >= CA is B's channel c - CA.
#ifndef SRK_DENSE_COMMON_H_
#define SRK_DENSE_COMMON_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/srk.h"

namespace srk {

constexpr int kDenseChan = 16;        // SRK_DENSE_CHANNEL_MULTIPLE: CA, CB and Cout are multiples of one MFMA tile edge
constexpr int kDenseMaxCout = 64;     // SRK_DENSE_MAX_COUT: four 16-channel accumulator tiles a wave
constexpr int kDensePixTile = 16;     // pixels of one MFMA tile (forward, data gradient)
constexpr int kDenseWgChunk = 32;     // pixels of one MFMA k-step of the weight gradient
constexpr int kDenseWavesWanted = 1024;               // forward / data gradient: one wave per SIMD of the part, at least
constexpr int kDenseWgWavesWanted = 2048;             // weight gradient: waves over (channel tile, tap, pixel split)
constexpr size_t kDenseWgMaxWs = (size_t)32 << 20;    // weight gradient: bytes of partials, at most

struct DensePlan {
  int pix_tiles;        // 16-pixel tiles a wave of the forward / data-gradient kernels owns: 1, 2 or 4
  int splits;           // pixel ranges of the weight gradient, reduced in index order
  int64_t split_pixels; // pixels per range (a multiple of kDenseWgChunk)
  size_t ws_bytes;      // splits * (Cout * (CA + CB) * K * K + Cout) floats
};

__host__ __device__ __forceinline__ int64_t dense_pixels(const srk_dense_desc& d) { return (int64_t)d.N * d.H * d.W; }
__host__ __device__ __forceinline__ int dense_ctot(const srk_dense_desc& d) { return d.CA + d.CB; }
// floats of one split's partials: dW in torch's order [Cout][CA + CB][K][K], then db [Cout]
__host__ __device__ __forceinline__ size_t dense_partial_floats(const srk_dense_desc& d) {
  return (size_t)d.Cout * dense_ctot(d) * d.K * d.K + (size_t)d.Cout;
}

// 0: fine.  Otherwise the status, *bad the offending number and *what its name.
__host__ __device__ inline int dense_check_desc(const srk_dense_desc& d, int* bad, const char** what) {
  auto fail = [&](int status, int v, const char* w) {
    *bad = v;
    *what = w;
    return status;
  };
  if (d.N <= 0) return fail(SRK_ERR_BAD_ARG, d.N, "N");
  if (d.H <= 0) return fail(SRK_ERR_BAD_ARG, d.H, "H");
  if (d.W <= 0) return fail(SRK_ERR_BAD_ARG, d.W, "W");
  if (d.CA <= 0) return fail(SRK_ERR_BAD_ARG, d.CA, "CA");
  if (d.CB < 0) return fail(SRK_ERR_BAD_ARG, d.CB, "CB");
  if (d.Cout <= 0) return fail(SRK_ERR_BAD_ARG, d.Cout, "Cout");
  if (d.terms != 3 && d.terms != 6) return fail(SRK_ERR_BAD_ARG, d.terms, "terms");
  if (d.act != SRK_ACT_NONE && d.act != SRK_ACT_RELU && d.act != SRK_ACT_LRELU) return fail(SRK_ERR_BAD_ARG, d.act, "act");
  if (d.K != 1 && d.K != 3) return fail(SRK_ERR_UNSUPPORTED, d.K, "K");
  if (d.CA % kDenseChan) return fail(SRK_ERR_UNSUPPORTED, d.CA, "CA");
  if (d.CB % kDenseChan) return fail(SRK_ERR_UNSUPPORTED, d.CB, "CB");
  if (d.Cout % kDenseChan || d.Cout > kDenseMaxCout) return fail(SRK_ERR_UNSUPPORTED, d.Cout, "Cout");
  if ((int64_t)d.N * d.H * d.W > (int64_t)1 << 30) return fail(SRK_ERR_UNSUPPORTED, d.N, "N * H * W");
  return SRK_OK;
}

// a slice's stride: at least its channels, and whole 16-byte groups (the kernels move four floats an access)
__host__ __device__ __forceinline__ bool dense_ld_ok(int ld, int C) { return ld >= C && ld % 4 == 0; }

__host__ __device__ inline DensePlan dense_plan(const srk_dense_desc& d) {
  DensePlan p;
  const int64_t P = dense_pixels(d);
  p.pix_tiles = P / 64 >= kDenseWavesWanted ? 4 : (P / 32 >= kDenseWavesWanted ? 2 : 1);
  const int64_t chunks = (P + kDenseWgChunk - 1) / kDenseWgChunk;
  const int64_t tiles = (int64_t)(dense_ctot(d) / kDenseChan) * d.K * d.K;
  int64_t want = (kDenseWgWavesWanted + tiles - 1) / tiles;
  const int64_t fit = (int64_t)(kDenseWgMaxWs / (dense_partial_floats(d) * sizeof(float)));
  if (want > fit) want = fit;
  if (want > chunks) want = chunks;
  if (want < 1) want = 1;
  const int64_t per = (chunks + want - 1) / want;
  p.splits = (int)((chunks + per - 1) / per);   // no empty range
  p.split_pixels = per * kDenseWgChunk;
  p.ws_bytes = (size_t)p.splits * dense_partial_floats(d) * sizeof(float);
  return p;
}

// pixel p -> (n, h, w)
__host__ __device__ __forceinline__ void dense_unflatten(int64_t p, int H, int W, int& n, int& h, int& w) {
  const int64_t hw = (int64_t)H * W;
  n = (int)(p / hw);
  const int r = (int)(p - (int64_t)n * hw);
  h = r / W;
  w = r - h * W;
}

// d act(v) / dv from the saved output (none: 1)
__host__ __device__ __forceinline__ float dense_act_grad(int act, float slope, float y_saved) {
  if (act == SRK_ACT_RELU) return y_saved > 0.f ? 1.f : 0.f;
  if (act == SRK_ACT_LRELU) return y_saved > 0.f ? 1.f : slope;
  return 1.f;
}

}  // namespace srk
#endif  // SRK_DENSE_COMMON_H_
