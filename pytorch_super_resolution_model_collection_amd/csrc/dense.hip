// Convolution over channel slices: y[.., slice] = act(conv([A | B]; W) + bias) (+ residual), its data gradient into two
// slices and its weight gradient.  Definition: include/srk.h and DESIGN.md 28; addressing and planner: dense_common.h,
// shared with the host twin at the end of this file.
//
//   forward          k_dense_fwd<NP, PT>     one block = 16 output channels x 4 waves of PT tiles of 16 pixels
//   data gradient    k_dense_dgrad<NP, PT>   one block = 64 input channels (grid.y walks [A | B]) x 4 waves of PT pixel tiles
//   weight gradient  k_dense_wgrad<NP>       one wave = 16 input channels x one tap x one pixel range -> partials
//                    k_dense_wreduce         the ranges added in index order, beta applied: dW and db
//   k_dense_fwd_ex / k_dense_dgrad_ex / k_dense_wgrad_ex: the same three bodies (dense_*_body<.., EX = true>) with the scaled
//                    output and the two scaled skips of srk_dense_epilogue -- the RRDB epilogues of ESRGAN, DESIGN.md 30
// All three products are v_mfma_f32_16x16x32_bf16 on split8n<NP> planes (bf16_frag.h): NP = 2 planes and three products
// (terms = 3), or NP = 3 planes and six (terms = 6), smallest products first as in k_conv_bfd.  Operand maps: A[row = lane &
// 15][k = 8 (lane >> 4) + j], B[k][col = lane & 15], D[row = 4 (lane >> 4) + reg][col = lane & 15].  The forward and the data
// gradient put the CHANNELS on the rows, so a lane's four results are four consecutive channels of one pixel: one 16-byte
// access for bias, residual, beta, add and the store.  The activations come straight from global memory -- a pixel's eight
// channels are 32 contiguous bytes of a slice whatever its stride; W is read in torch's order and staged through LDS by the
// block that uses it, so nothing is packed and a layer is one launch.  No atomics anywhere.
#include <math.h>

#include <vector>

#include "bf16_frag.h"
#include "dense_common.h"
#include "srk_common.h"

namespace srk {

// srk_dense_epilogue as the _ex kernels take it
struct DenseEpi {
  float s = 1.f, r1 = 1.f, r2 = 0.f, a1 = 1.f;
  const float* R2 = nullptr;
  int ldR2 = 0;
};

template <int NP>
__device__ __forceinline__ f32x4 dense_mma(const uint4 (&a)[NP], const uint4 (&b)[NP], f32x4 c) {
  if constexpr (NP == 3) {
    c = mfma16(a[2], b[0], c);
    c = mfma16(a[0], b[2], c);
    c = mfma16(a[1], b[1], c);
  }
  c = mfma16(a[1], b[0], c);
  c = mfma16(a[0], b[1], c);
  return mfma16(a[0], b[0], c);
}

__device__ __forceinline__ void dense_load8(const float* p, float (&f)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) f[e] = a[e], f[4 + e] = b[e];
}

__device__ __forceinline__ float dense_mask(int act, float slope, float g, float y_saved) {
  if (act == SRK_ACT_RELU) return y_saved > 0.f ? g : 0.f;
  if (act == SRK_ACT_LRELU) return y_saved > 0.f ? g : slope * g;
  return g;
}

// pixel (n, h + dh, w + dw) of the image, or -1 outside it
__device__ __forceinline__ int dense_neighbour(int n, int h, int w, int dh, int dw, int H, int W) {
  const int hh = h + dh, ww = w + dw;
  return ((unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W) ? (n * H + hh) * W + ww : -1;
}

// Filters reach the MFMAs through LDS: read as torch stores them, a lane's eight filter values lie K K floats apart and the
// 16 lanes of a row (CA + CB) K K floats apart, 64 cache lines a load instruction, and the first version of these kernels was
// bound by the L1's line rate at 2 % of the matrix peak.  The 32 channels x K K taps of one output channel are
// contiguous, so a block copies them with consecutive lanes on consecutive floats and its four waves pick their fragments
// out of LDS.  Row pitch odd: the 16 lanes of one quarter-wave (one q) hit 16 different banks.  The four quarters are NOT
// kept apart -- a lane reads bank (33 col + 8 q K K + ...) mod 64, so (col 8, q 0) meets (col 0, q 1): a 64-lane read has
// conflicts, about 2-way.  Not measured and not tuned.
constexpr int kDenseFwdPitch = 32 * 9 + 1;          // floats of one output channel's 32 x K K filter row in LDS
constexpr int kDenseDgPitch = 64 * 9 + 1;           // floats of one output channel's 64-input-channel row (data gradient)

// One block = ONE tile of 16 output channels x four pixel groups, one a wave, of PT tiles of 16 pixels.  Per chunk of 32
// input channels the block stages W[16 oc][32 ic][K K] once; every wave then walks the taps.
// The body is shared by k_dense_fwd and k_dense_fwd_ex (EX: the scaled output and the two scaled skips of DenseEpi).
template <int NP, int PT, bool EX>
__device__ __forceinline__ void dense_fwd_body(const srk_dense_desc& d, const float* A, const float* B, const float* Wt,
                                               const float* bias, const float* res, float* y, int P, const DenseEpi& e,
                                               float* sw) {
  const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
  const int OT = d.Cout >> 4;
  const int o = blockIdx.x % OT;
  const int64_t p64 = ((int64_t)(blockIdx.x / OT) * 4 + (threadIdx.x >> 6)) * (PT * kDensePixTile);
  const bool alive = p64 < P;       // (a wave past the end still stages filters and meets the barriers)
  const int p0 = alive ? (int)p64 : 0;
  const int Ctot = d.CA + d.CB, KK = d.K * d.K, pad = d.K >> 1;
  int pn[PT], ph[PT], pw[PT];
  bool pv[PT];
#pragma unroll
  for (int t = 0; t < PT; ++t) {
    const int p = p0 + t * kDensePixTile + col;
    pv[t] = alive && p < P;
    dense_unflatten(pv[t] ? p : 0, d.H, d.W, pn[t], ph[t], pw[t]);
  }
  f32x4 acc[PT];
#pragma unroll
  for (int t = 0; t < PT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int RL = 32 * KK;           // floats of a staged row
  for (int c0 = 0; c0 < Ctot; c0 += 32) {
    const int nvalid = (Ctot - c0 < 32 ? Ctot - c0 : 32) * KK;
    __syncthreads();                // the previous chunk's fragment reads are done
    for (int idx = threadIdx.x; idx < 16 * RL; idx += 256) {
      const int r = idx / RL, e = idx - r * RL;
      sw[r * kDenseFwdPitch + e] = e < nvalid ? Wt[((size_t)(o * 16 + r) * Ctot + c0) * KK + e] : 0.f;
    }
    __syncthreads();
    if (!alive) continue;
    const int c = c0 + 8 * q;       // this lane's eight input channels; a group of 8 never straddles A | B
    const bool cv = c < Ctot;
    for (int tap = 0; tap < KK; ++tap) {
      const int dh = tap / d.K - pad, dw = tap % d.K - pad;
      uint4 wa[NP], xb[PT][NP];
      {
        float f[8];
        const float* wp = sw + col * kDenseFwdPitch + 8 * q * KK + tap;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = wp[j * KK];
        split8n<NP>(f, wa);
      }
#pragma unroll
      for (int t = 0; t < PT; ++t) {
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int pix = (cv && pv[t]) ? dense_neighbour(pn[t], ph[t], pw[t], dh, dw, d.H, d.W) : -1;
        if (pix >= 0) dense_load8(c < d.CA ? A + (size_t)pix * d.ldA + c : B + (size_t)pix * d.ldB + (c - d.CA), f);
        split8n<NP>(f, xb[t]);
      }
#pragma unroll
      for (int t = 0; t < PT; ++t) acc[t] = dense_mma<NP>(wa, xb[t], acc[t]);
    }
  }
  if (!alive) return;
  const int oc = o * 16 + q * 4;
  f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
  if (bias) bv = *reinterpret_cast<const f32x4*>(bias + oc);
#pragma unroll
  for (int t = 0; t < PT; ++t) {
    const int p = p0 + t * kDensePixTile + col;
    if (p >= P) continue;
    f32x4 v = acc[t] + bv;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = act_apply(v[e], d.act, d.slope);
    if constexpr (EX) {
      v *= e.s;
      if (res) v += e.r1 * *reinterpret_cast<const f32x4*>(res + (size_t)p * d.ldR + oc);
      if (e.R2) v += e.r2 * *reinterpret_cast<const f32x4*>(e.R2 + (size_t)p * e.ldR2 + oc);
    } else {
      if (res) v += *reinterpret_cast<const f32x4*>(res + (size_t)p * d.ldR + oc);
    }
    *reinterpret_cast<f32x4*>(y + (size_t)p * d.ldY + oc) = v;
  }
}

template <int NP, int PT>
__global__ __launch_bounds__(256) void k_dense_fwd(srk_dense_desc d, const float* A, const float* B, const float* Wt,
                                                   const float* bias, const float* res, float* y, int P) {
  __shared__ float sw[16 * kDenseFwdPitch];
  dense_fwd_body<NP, PT, false>(d, A, B, Wt, bias, res, y, P, DenseEpi{}, sw);
}

template <int NP, int PT>
__global__ __launch_bounds__(256) void k_dense_fwd_ex(srk_dense_desc d, const float* A, const float* B, const float* Wt,
                                                      const float* bias, const float* res, float* y, int P, DenseEpi e) {
  __shared__ float sw[16 * kDenseFwdPitch];
  dense_fwd_body<NP, PT, true>(d, A, B, Wt, bias, res, y, P, e, sw);
}

// dX[p][ic] = sum over taps, oc of g[p - (tap - pad)][oc] * W[oc][ic][tap].  One block = up to four tiles of 16 input
// channels (blockIdx.y: which 64 channels of [A | B]) x four pixel groups, one a wave, so a g fragment -- two slices read
// and a mask -- serves four products.  Per chunk of 32 output channels the block stages W[32 oc][64 ic][K K] (dynamic LDS,
// 32 rows of kDenseDgPitch floats) once; every wave then walks the taps.
// EX (k_dense_dgrad_ex): g is scaled by e.s where it is read and `add` by e.a1.
template <int NP, int PT, bool EX>
__device__ __forceinline__ void dense_dgrad_body(const srk_dense_desc& d, const float* dy, const float* ys, const float* Wt,
                                                 float* dA, float betaA, float* dB, float betaB, const float* add, int P,
                                                 const DenseEpi& e, float* sdw) {
  const int lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
  const int64_t p64 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (PT * kDensePixTile);
  const bool alive = p64 < P;
  const int p0 = alive ? (int)p64 : 0;
  const int Ctot = d.CA + d.CB, KK = d.K * d.K, pad = d.K >> 1;
  const int ic0 = blockIdx.y * 64;
  const int OT = (Ctot - ic0) >= 64 ? 4 : (Ctot - ic0) >> 4;
  const bool masked = d.act != SRK_ACT_NONE;
  int pn[PT], ph[PT], pw[PT];
  bool pv[PT];
#pragma unroll
  for (int t = 0; t < PT; ++t) {
    const int p = p0 + t * kDensePixTile + col;
    pv[t] = alive && p < P;
    dense_unflatten(pv[t] ? p : 0, d.H, d.W, pn[t], ph[t], pw[t]);
  }
  f32x4 acc[4][PT];
#pragma unroll
  for (int o = 0; o < 4; ++o)
#pragma unroll
    for (int t = 0; t < PT; ++t) acc[o][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int RL = OT * 16 * KK;      // floats of a staged row: this block's input channels x taps of one output channel
  for (int c0 = 0; c0 < d.Cout; c0 += 32) {
    const int rows = d.Cout - c0 < 32 ? d.Cout - c0 : 32;
    __syncthreads();
    for (int idx = threadIdx.x; idx < 32 * RL; idx += 256) {
      const int r = idx / RL, e = idx - r * RL;
      sdw[r * kDenseDgPitch + e] = r < rows ? Wt[((size_t)(c0 + r) * Ctot + ic0) * KK + e] : 0.f;
    }
    __syncthreads();
    if (!alive) continue;
    const int c = c0 + 8 * q;       // this lane's eight output channels
    const bool cv = c < d.Cout;
    for (int tap = 0; tap < KK; ++tap) {
      const int dh = pad - tap / d.K, dw = pad - tap % d.K;
      uint4 wa[4][NP], gb[PT][NP];
#pragma unroll
      for (int o = 0; o < 4; ++o)
        if (o < OT) {
          float f[8];
          const float* wp = sdw + 8 * q * kDenseDgPitch + (o * 16 + col) * KK + tap;
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = wp[j * kDenseDgPitch];
          split8n<NP>(f, wa[o]);
        }
#pragma unroll
      for (int t = 0; t < PT; ++t) {
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int pix = (cv && pv[t]) ? dense_neighbour(pn[t], ph[t], pw[t], dh, dw, d.H, d.W) : -1;
        if (pix >= 0) {
          dense_load8(dy + (size_t)pix * d.ldDy + c, f);
          if (masked) {
            float m[8];
            dense_load8(ys + (size_t)pix * d.ldY + c, m);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = dense_mask(d.act, d.slope, f[j], m[j]);
          }
          if constexpr (EX) {
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] *= e.s;
          }
        }
        split8n<NP>(f, gb[t]);
      }
#pragma unroll
      for (int o = 0; o < 4; ++o)
        if (o < OT) {
#pragma unroll
          for (int t = 0; t < PT; ++t) acc[o][t] = dense_mma<NP>(wa[o], gb[t], acc[o][t]);
        }
    }
  }
  if (!alive) return;
#pragma unroll
  for (int o = 0; o < 4; ++o)
    if (o < OT) {
      const int ic = ic0 + o * 16 + q * 4;      // a tile of 16 lies in A or in B
      const bool inA = ic < d.CA;
      float* dst = inA ? dA : dB;
      if (!dst) continue;
      const int ld = inA ? d.ldDA : d.ldDB, off = inA ? ic : ic - d.CA;
      const float beta = inA ? betaA : betaB;
#pragma unroll
      for (int t = 0; t < PT; ++t) {
        const int p = p0 + t * kDensePixTile + col;
        if (p >= P) continue;
        f32x4 v = acc[o][t];
        if (inA && add) {
          const f32x4 av = *reinterpret_cast<const f32x4*>(add + (size_t)p * d.ldAdd + ic);
          if constexpr (EX) v += e.a1 * av; else v += av;
        }
        f32x4* out = reinterpret_cast<f32x4*>(dst + (size_t)p * ld + off);
        if (beta != 0.f) v += *out;   // (beta == 0: the destination may hold anything)
        *out = v;
      }
    }
}

template <int NP, int PT>
__global__ __launch_bounds__(256) void k_dense_dgrad(srk_dense_desc d, const float* dy, const float* ys, const float* Wt,
                                                     float* dA, float betaA, float* dB, float betaB, const float* add, int P) {
  extern __shared__ float sdw[];
  dense_dgrad_body<NP, PT, false>(d, dy, ys, Wt, dA, betaA, dB, betaB, add, P, DenseEpi{}, sdw);
}

template <int NP, int PT>
__global__ __launch_bounds__(256) void k_dense_dgrad_ex(srk_dense_desc d, const float* dy, const float* ys, const float* Wt,
                                                        float* dA, float betaA, float* dB, float betaB, const float* add,
                                                        int P, DenseEpi e) {
  extern __shared__ float sdw[];
  dense_dgrad_body<NP, PT, true>(d, dy, ys, Wt, dA, betaA, dB, betaB, add, P, e, sdw);
}

// partial[split][oc][ic][tap] = sum over the range's pixels of g[p][oc] * X[p + tap - pad][ic]; the (tile 0, tap 0) wave of
// a range also leaves sum_p g[p][oc] (a product with a plane of ones) behind the range's dW partials.
// blockIdx.x = (input-channel tile) * K * K + tap, blockIdx.y = range.  The next 32 pixels' raw operands are requested
// before this chunk's MFMAs.
// EX (k_dense_wgrad_ex): g is scaled by gs where it is read.
template <int NP, bool EX>
__device__ __forceinline__ void dense_wgrad_body(const srk_dense_desc& d, const float* A, const float* B, const float* dy,
                                                 const float* ys, float* ws, int P, int split_pixels, float gs) {
  const int lane = threadIdx.x, col = lane & 15, q = lane >> 4;
  const int Ctot = d.CA + d.CB, KK = d.K * d.K, pad = d.K >> 1, OT = d.Cout >> 4;
  const int it = blockIdx.x / KK, tap = blockIdx.x - it * KK;
  const int dh = tap / d.K - pad, dw = tap % d.K - pad;
  const int64_t pb64 = (int64_t)blockIdx.y * split_pixels;
  const int pbeg = (int)(pb64 < P ? pb64 : P);
  const int pend = pbeg + split_pixels < P ? pbeg + split_pixels : P;
  const bool do_bias = blockIdx.x == 0;
  const bool masked = d.act != SRK_ACT_NONE;
  const int ic = it * 16 + col;
  const float* src = ic < d.CA ? A + ic : B + (ic - d.CA);
  const int lds = ic < d.CA ? d.ldA : d.ldB;
  uint4 ones;
  ones.x = ones.y = ones.z = ones.w = 0x3f803f80u;   // eight bf16 1.0
  f32x4 acc[4], accb[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) acc[o] = accb[o] = f32x4{0.f, 0.f, 0.f, 0.f};
  float xf[8], gf[4][8], mf[4][8];
  auto load = [&](int pc) {
    const int pl = pc + 8 * q;      // this lane's eight pixels of the chunk
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int p = pl + j;
      xf[j] = 0.f;
#pragma unroll
      for (int o = 0; o < 4; ++o) gf[o][j] = 0.f, mf[o][j] = 1.f;
      if (p >= pend) continue;
      int pp = p;
      if (d.K != 1) {
        int n, h, w;
        dense_unflatten(p, d.H, d.W, n, h, w);
        pp = dense_neighbour(n, h, w, dh, dw, d.H, d.W);
      }
      if (pp >= 0) xf[j] = src[(size_t)pp * lds];
#pragma unroll
      for (int o = 0; o < 4; ++o)
        if (o < OT) {
          gf[o][j] = dy[(size_t)p * d.ldDy + o * 16 + col];
          if (masked) mf[o][j] = ys[(size_t)p * d.ldY + o * 16 + col];
        }
    }
  };
  if (pbeg < pend) load(pbeg);
  for (int pc = pbeg; pc < pend; pc += kDenseWgChunk) {
    uint4 xb[NP], ga[4][NP];
    split8n<NP>(xf, xb);
#pragma unroll
    for (int o = 0; o < 4; ++o)
      if (o < OT) {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          f[j] = dense_mask(d.act, d.slope, gf[o][j], mf[o][j]);
          if constexpr (EX) f[j] *= gs;
        }
        split8n<NP>(f, ga[o]);
      }
    if (pc + kDenseWgChunk < pend) load(pc + kDenseWgChunk);
#pragma unroll
    for (int o = 0; o < 4; ++o)
      if (o < OT) {
        acc[o] = dense_mma<NP>(ga[o], xb, acc[o]);
        if (do_bias) {
#pragma unroll
          for (int k = NP - 1; k >= 0; --k) accb[o] = mfma16(ga[o][k], ones, accb[o]);
        }
      }
  }
  float* part = ws + (size_t)blockIdx.y * dense_partial_floats(d);
#pragma unroll
  for (int o = 0; o < 4; ++o)
    if (o < OT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int oc = o * 16 + q * 4 + r;
        part[((size_t)oc * Ctot + ic) * KK + tap] = acc[o][r];
        if (do_bias && col == 0) part[(size_t)d.Cout * Ctot * KK + oc] = accb[o][r];
      }
    }
}

template <int NP>
__global__ __launch_bounds__(64) void k_dense_wgrad(srk_dense_desc d, const float* A, const float* B, const float* dy,
                                                    const float* ys, float* ws, int P, int split_pixels) {
  dense_wgrad_body<NP, false>(d, A, B, dy, ys, ws, P, split_pixels, 1.f);
}

template <int NP>
__global__ __launch_bounds__(64) void k_dense_wgrad_ex(srk_dense_desc d, const float* A, const float* B, const float* dy,
                                                       const float* ys, float* ws, int P, int split_pixels, float gs) {
  dense_wgrad_body<NP, true>(d, A, B, dy, ys, ws, P, split_pixels, gs);
}

__global__ __launch_bounds__(256) void k_dense_wreduce(const float* __restrict__ ws, int splits, size_t partial_floats,
                                                       size_t nw, float* __restrict__ dW, float* __restrict__ db,
                                                       float beta) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= partial_floats) return;
  float* out = i < nw ? (dW ? dW + i : nullptr) : (db ? db + (i - nw) : nullptr);
  if (!out) return;
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += ws[(size_t)k * partial_floats + i];
  *out = beta == 0.f ? s : *out + s;   // (beta == 0: the destination may hold anything)
}

static int dense_check(const srk_dense_desc* d, const char* who) {
  SRK_REQUIRE(d, "%s: null descriptor", who);
  int bad = 0;
  const char* what = "";
  const int rc = dense_check_desc(*d, &bad, &what);
  if (rc == SRK_ERR_UNSUPPORTED)
    set_error("%s: %s = %d is not supported (K in {1, 3}; CA, CB, Cout multiples of %d; Cout <= %d)", who, what, bad,
              kDenseChan, kDenseMaxCout);
  else if (rc)
    set_error("%s: bad %s = %d", who, what, bad);
  return rc;
}

static int dense_check_ld(const char* who, const char* name, int ld, int C) {
  if (ld < C) {
    set_error("%s: %s = %d is smaller than the slice's %d channels", who, name, ld, C);
    return SRK_ERR_BAD_ARG;
  }
  if (ld % 4) {
    set_error("%s: %s = %d is not supported (pixel strides are multiples of 4 floats)", who, name, ld);
    return SRK_ERR_UNSUPPORTED;
  }
  return SRK_OK;
}

template <typename... P>
static int dense_check_align(const char* who, const P*... p) {
  if (!aligned16(p...)) {
    set_error("%s: a slice pointer is not 16-byte aligned (channel offsets are multiples of 4)", who);
    return SRK_ERR_UNSUPPORTED;
  }
  return SRK_OK;
}

static int dense_check_beta(const char* who, float beta) {
  SRK_REQUIRE(beta == 0.f || beta == 1.f, "%s: beta = %g is neither 0 nor 1", who, (double)beta);
  return SRK_OK;
}

// the caller's epilogue (NULL: the plain operator) as the kernels take it
static int dense_epilogue(const char* who, const srk_dense_epilogue* e, const float* R2, DenseEpi* out) {
  *out = DenseEpi{};
  if (!e) {
    SRK_REQUIRE(!R2, "%s: R2 needs an epilogue (its scale and pixel stride)", who);
    return SRK_OK;
  }
  SRK_REQUIRE(e->struct_size >= sizeof(srk_dense_epilogue), "%s: the epilogue's struct_size = %u is too small", who,
              (unsigned)e->struct_size);
  SRK_REQUIRE(isfinite(e->s) && isfinite(e->r1) && isfinite(e->r2) && isfinite(e->a1),
              "%s: an epilogue scale is not finite (s = %g, r1 = %g, r2 = %g, a1 = %g)", who, (double)e->s, (double)e->r1,
              (double)e->r2, (double)e->a1);
  out->s = e->s, out->r1 = e->r1, out->r2 = e->r2, out->a1 = e->a1;
  out->R2 = R2, out->ldR2 = e->ldR2;
  return SRK_OK;
}

}  // namespace srk

using namespace srk;

extern "C" int srk_dense_conv_supported(const srk_dense_desc* d) {
  if (!d) return 0;
  int bad = 0;
  const char* what = "";
  if (dense_check_desc(*d, &bad, &what)) return 0;
  return dense_ld_ok(d->ldA, d->CA) && (d->CB == 0 || dense_ld_ok(d->ldB, d->CB)) && dense_ld_ok(d->ldY, d->Cout);
}

extern "C" int srk_dense_conv_plan(const srk_dense_desc* d, srk_dense_plan* plan) {
  const char* who = "dense_conv_plan";
  if (int rc = dense_check(d, who)) return rc;
  SRK_REQUIRE(plan && plan->struct_size >= sizeof(srk_dense_plan), "%s: plan is null or its struct_size is too small", who);
  const DensePlan p = dense_plan(*d);
  plan->pix_tiles = p.pix_tiles;
  plan->splits = p.splits;
  plan->split_pixels = p.split_pixels;
  plan->ws_bytes = p.ws_bytes;
  plan->partial_floats = dense_partial_floats(*d);
  return SRK_OK;
}

extern "C" size_t srk_dense_conv_workspace_bytes(const srk_dense_desc* d) {
  if (dense_check(d, "dense_conv_workspace_bytes")) return 0;
  return dense_plan(*d).ws_bytes;
}

// ex: the _ex entry point (its kernels, whatever the scales); else the kernels RDN has always run
static int dense_forward(const char* who, bool ex, const srk_dense_desc* d, const float* A, const float* B, const float* W,
                         const float* bias, const float* residual, const float* R2, const srk_dense_epilogue* epi, float* y,
                         void* stream) {
  if (int rc = dense_check(d, who)) return rc;
  DenseEpi e;
  if (int rc = dense_epilogue(who, epi, R2, &e)) return rc;
  if (R2)
    if (int rc = dense_check_ld(who, "ldR2", e.ldR2, d->Cout)) return rc;
  SRK_REQUIRE(A && W && y && (B || d->CB == 0), "%s: null pointer", who);
  if (int rc = dense_check_ld(who, "ldA", d->ldA, d->CA)) return rc;
  if (d->CB)
    if (int rc = dense_check_ld(who, "ldB", d->ldB, d->CB)) return rc;
  if (int rc = dense_check_ld(who, "ldY", d->ldY, d->Cout)) return rc;
  if (residual)
    if (int rc = dense_check_ld(who, "ldR", d->ldR, d->Cout)) return rc;
  if (int rc = dense_check_align(who, A, d->CB ? B : nullptr, bias, residual, R2, (const float*)y)) return rc;
  const DensePlan pl = dense_plan(*d);
  const int P = (int)dense_pixels(*d);
  const dim3 grid(cdiv(cdiv((size_t)P, (size_t)pl.pix_tiles * kDensePixTile), 4) * (unsigned)(d->Cout / kDenseChan)), blk(256);
  hipStream_t st = (hipStream_t)stream;
  if (d->CB == 0) B = A;   // never read
#define SRK_DENSE_FWD(NP, PT)                                                                              \
  do {                                                                                                     \
    if (ex) hipLaunchKernelGGL((k_dense_fwd_ex<NP, PT>), grid, blk, 0, st, *d, A, B, W, bias, residual, y, P, e); \
    else hipLaunchKernelGGL((k_dense_fwd<NP, PT>), grid, blk, 0, st, *d, A, B, W, bias, residual, y, P);   \
  } while (0)
  if (d->terms == 6) {
    if (pl.pix_tiles == 4) SRK_DENSE_FWD(3, 4); else if (pl.pix_tiles == 2) SRK_DENSE_FWD(3, 2); else SRK_DENSE_FWD(3, 1);
  } else {
    if (pl.pix_tiles == 4) SRK_DENSE_FWD(2, 4); else if (pl.pix_tiles == 2) SRK_DENSE_FWD(2, 2); else SRK_DENSE_FWD(2, 1);
  }
#undef SRK_DENSE_FWD
  note_kernel(ex ? "k_dense_fwd_ex<%d,%d>" : "k_dense_fwd<%d,%d>", d->terms == 6 ? 3 : 2, pl.pix_tiles);
  return check_launch(who);
}

extern "C" int srk_dense_conv_forward(const srk_dense_desc* d, const float* A, const float* B, const float* W,
                                      const float* bias, const float* residual, float* y, void* stream) {
  return dense_forward("dense_conv_forward", false, d, A, B, W, bias, residual, nullptr, nullptr, y, stream);
}

extern "C" int srk_dense_conv_forward_ex(const srk_dense_desc* d, const float* A, const float* B, const float* W,
                                         const float* bias, const float* R1, const float* R2, const srk_dense_epilogue* e,
                                         float* y, void* stream) {
  return dense_forward("dense_conv_forward_ex", true, d, A, B, W, bias, R1, R2, e, y, stream);
}

static int dense_backward_data(const char* who, bool ex, const srk_dense_desc* d, const float* dy, const float* y_saved,
                               const float* W, float* dA, float betaA, float* dB, float betaB, const float* add,
                               const srk_dense_epilogue* epi, void* stream) {
  if (int rc = dense_check(d, who)) return rc;
  DenseEpi e;
  if (int rc = dense_epilogue(who, epi, nullptr, &e)) return rc;
  SRK_REQUIRE(dy && W && (dA || dB), "%s: null pointer", who);
  SRK_REQUIRE(y_saved || d->act == SRK_ACT_NONE, "%s: an activation needs the saved output", who);
  SRK_REQUIRE(!add || dA, "%s: add goes into dA, which is null", who);
  if (d->CB == 0) dB = nullptr;
  if (int rc = dense_check_beta(who, betaA)) return rc;
  if (int rc = dense_check_beta(who, betaB)) return rc;
  if (int rc = dense_check_ld(who, "ldDy", d->ldDy, d->Cout)) return rc;
  if (y_saved && d->act != SRK_ACT_NONE)
    if (int rc = dense_check_ld(who, "ldY", d->ldY, d->Cout)) return rc;
  if (dA)
    if (int rc = dense_check_ld(who, "ldDA", d->ldDA, d->CA)) return rc;
  if (dB)
    if (int rc = dense_check_ld(who, "ldDB", d->ldDB, d->CB)) return rc;
  if (add)
    if (int rc = dense_check_ld(who, "ldAdd", d->ldAdd, d->CA)) return rc;
  if (int rc = dense_check_align(who, dy, d->act != SRK_ACT_NONE ? y_saved : nullptr, (const float*)dA, (const float*)dB, add))
    return rc;
  const DensePlan pl = dense_plan(*d);
  const int P = (int)dense_pixels(*d);
  const dim3 grid(cdiv(cdiv((size_t)P, (size_t)pl.pix_tiles * kDensePixTile), 4), cdiv((size_t)dense_ctot(*d), 64)), blk(256);
  hipStream_t st = (hipStream_t)stream;
#define SRK_DENSE_DG(NP, PT)                                                                                          \
  do {                                                                                                                \
    if (ex) launch_lds<k_dense_dgrad_ex<NP, PT>>(grid, blk, (size_t)32 * kDenseDgPitch * sizeof(float), st, *d, dy, y_saved, W, dA, betaA, dB, betaB, add, P, e); \
    else launch_lds<k_dense_dgrad<NP, PT>>(grid, blk, (size_t)32 * kDenseDgPitch * sizeof(float), st, *d, dy, y_saved, W, dA, betaA, dB, betaB, add, P); \
  } while (0)
  if (d->terms == 6) {
    if (pl.pix_tiles == 4) SRK_DENSE_DG(3, 4); else if (pl.pix_tiles == 2) SRK_DENSE_DG(3, 2); else SRK_DENSE_DG(3, 1);
  } else {
    if (pl.pix_tiles == 4) SRK_DENSE_DG(2, 4); else if (pl.pix_tiles == 2) SRK_DENSE_DG(2, 2); else SRK_DENSE_DG(2, 1);
  }
#undef SRK_DENSE_DG
  note_kernel(ex ? "k_dense_dgrad_ex<%d,%d>" : "k_dense_dgrad<%d,%d>", d->terms == 6 ? 3 : 2, pl.pix_tiles);
  return check_launch(who);
}

extern "C" int srk_dense_conv_backward_data(const srk_dense_desc* d, const float* dy, const float* y_saved, const float* W,
                                            float* dA, float betaA, float* dB, float betaB, const float* add, void* stream) {
  return dense_backward_data("dense_conv_backward_data", false, d, dy, y_saved, W, dA, betaA, dB, betaB, add, nullptr, stream);
}

extern "C" int srk_dense_conv_backward_data_ex(const srk_dense_desc* d, const float* dy, const float* y_saved, const float* W,
                                               float* dA, float betaA, float* dB, float betaB, const float* add,
                                               const srk_dense_epilogue* e, void* stream) {
  return dense_backward_data("dense_conv_backward_data_ex", true, d, dy, y_saved, W, dA, betaA, dB, betaB, add, e, stream);
}

static int dense_backward_weight(const char* who, bool ex, const srk_dense_desc* d, const float* A, const float* B,
                                 const float* dy, const float* y_saved, float* dW, float* db, float beta,
                                 const srk_dense_epilogue* epi, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = dense_check(d, who)) return rc;
  DenseEpi e;
  if (int rc = dense_epilogue(who, epi, nullptr, &e)) return rc;
  SRK_REQUIRE(A && dy && (dW || db) && workspace && (B || d->CB == 0), "%s: null pointer", who);
  SRK_REQUIRE(y_saved || d->act == SRK_ACT_NONE, "%s: an activation needs the saved output", who);
  if (int rc = dense_check_beta(who, beta)) return rc;
  if (int rc = dense_check_ld(who, "ldA", d->ldA, d->CA)) return rc;
  if (d->CB)
    if (int rc = dense_check_ld(who, "ldB", d->ldB, d->CB)) return rc;
  if (int rc = dense_check_ld(who, "ldDy", d->ldDy, d->Cout)) return rc;
  if (y_saved && d->act != SRK_ACT_NONE)
    if (int rc = dense_check_ld(who, "ldY", d->ldY, d->Cout)) return rc;
  const DensePlan pl = dense_plan(*d);
  if (workspace_bytes < pl.ws_bytes) {
    set_error("%s: workspace of %zu bytes, srk_dense_conv_workspace_bytes says %zu", who, workspace_bytes, pl.ws_bytes);
    return SRK_ERR_WORKSPACE;
  }
  const int P = (int)dense_pixels(*d);
  const int KK = d->K * d->K, Ctot = dense_ctot(*d);
  const dim3 grid((unsigned)(Ctot / kDenseChan * KK), (unsigned)pl.splits), blk(64);
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  if (d->CB == 0) B = A;   // never read
  if (ex) {
    if (d->terms == 6)
      hipLaunchKernelGGL(k_dense_wgrad_ex<3>, grid, blk, 0, st, *d, A, B, dy, y_saved, ws, P, (int)pl.split_pixels, e.s);
    else
      hipLaunchKernelGGL(k_dense_wgrad_ex<2>, grid, blk, 0, st, *d, A, B, dy, y_saved, ws, P, (int)pl.split_pixels, e.s);
  } else if (d->terms == 6)
    hipLaunchKernelGGL(k_dense_wgrad<3>, grid, blk, 0, st, *d, A, B, dy, y_saved, ws, P, (int)pl.split_pixels);
  else
    hipLaunchKernelGGL(k_dense_wgrad<2>, grid, blk, 0, st, *d, A, B, dy, y_saved, ws, P, (int)pl.split_pixels);
  const size_t pf = dense_partial_floats(*d);
  hipLaunchKernelGGL(k_dense_wreduce, dim3(cdiv(pf, 256)), dim3(256), 0, st, (const float*)ws, pl.splits, pf,
                     pf - (size_t)d->Cout, dW, db, beta);
  note_kernel(ex ? "k_dense_wgrad_ex<%d> x%d" : "k_dense_wgrad<%d> x%d", d->terms == 6 ? 3 : 2, pl.splits);
  return check_launch(who);
}

extern "C" int srk_dense_conv_backward_weight(const srk_dense_desc* d, const float* A, const float* B, const float* dy,
                                              const float* y_saved, float* dW, float* db, float beta, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  return dense_backward_weight("dense_conv_backward_weight", false, d, A, B, dy, y_saved, dW, db, beta, nullptr, workspace,
                               workspace_bytes, stream);
}

extern "C" int srk_dense_conv_backward_weight_ex(const srk_dense_desc* d, const float* A, const float* B, const float* dy,
                                                 const float* y_saved, float* dW, float* db, float beta,
                                                 const srk_dense_epilogue* e, void* workspace, size_t workspace_bytes,
                                                 void* stream) {
  return dense_backward_weight("dense_conv_backward_weight_ex", true, d, A, B, dy, y_saved, dW, db, beta, e, workspace,
                               workspace_bytes, stream);
}

// The same three directions as plain loops over host pointers, fp64 accumulation, one rounding to fp32 at the store.
static int dense_host(const char* who, const srk_dense_desc* dp, int direction, const float* A, const float* B, const float* W,
                      const float* bias, const float* residual, const float* R2, const srk_dense_epilogue* epi, float* y,
                      const float* dy, const float* add, float* dA, float betaA, float* dB, float betaB, float* dW, float* db,
                      float beta) {
  if (int rc = dense_check(dp, who)) return rc;
  const srk_dense_desc& d = *dp;
  DenseEpi e;
  if (int rc = dense_epilogue(who, epi, R2, &e)) return rc;
  SRK_REQUIRE(direction >= 0 && direction <= 2, "%s: direction %d is not 0 (forward), 1 (data) or 2 (weight)", who, direction);
  const int Ctot = dense_ctot(d), K = d.K, KK = K * K, pad = K >> 1;
  const int64_t P = dense_pixels(d);
  auto src = [&](int64_t pix, int c) -> float {
    return c < d.CA ? A[(size_t)pix * d.ldA + c] : B[(size_t)pix * d.ldB + (c - d.CA)];
  };
  auto neighbour = [&](int64_t p, int dh, int dw) -> int64_t {
    int n, h, w;
    dense_unflatten(p, d.H, d.W, n, h, w);
    const int hh = h + dh, ww = w + dw;
    return (hh >= 0 && hh < d.H && ww >= 0 && ww < d.W) ? ((int64_t)n * d.H + hh) * d.W + ww : -1;
  };
  auto grad = [&](int64_t p, int oc) -> double {   // g = s * dy * act'(y_saved)
    const double g = (double)e.s * (double)dy[(size_t)p * d.ldDy + oc];
    if (d.act == SRK_ACT_NONE) return g;
    return g * (double)dense_act_grad(d.act, d.slope, y[(size_t)p * d.ldY + oc]);
  };
  if (direction == 0) {
    SRK_REQUIRE(A && W && y && (B || d.CB == 0), "%s: null pointer", who);
    if (int rc = dense_check_ld(who, "ldA", d.ldA, d.CA)) return rc;
    if (d.CB)
      if (int rc = dense_check_ld(who, "ldB", d.ldB, d.CB)) return rc;
    if (int rc = dense_check_ld(who, "ldY", d.ldY, d.Cout)) return rc;
    if (residual)
      if (int rc = dense_check_ld(who, "ldR", d.ldR, d.Cout)) return rc;
    if (R2)
      if (int rc = dense_check_ld(who, "ldR2", e.ldR2, d.Cout)) return rc;
    for (int64_t p = 0; p < P; ++p)
      for (int oc = 0; oc < d.Cout; ++oc) {
        double a = bias ? (double)bias[oc] : 0.0;
        for (int tap = 0; tap < KK; ++tap) {
          const int64_t pp = neighbour(p, tap / K - pad, tap % K - pad);
          if (pp < 0) continue;
          for (int c = 0; c < Ctot; ++c) a += (double)src(pp, c) * (double)W[((size_t)oc * Ctot + c) * KK + tap];
        }
        if (d.act == SRK_ACT_RELU) a = a > 0.0 ? a : 0.0;
        if (d.act == SRK_ACT_LRELU) a = a > 0.0 ? a : (double)d.slope * a;
        a *= (double)e.s;
        if (residual) a += (double)e.r1 * (double)residual[(size_t)p * d.ldR + oc];
        if (R2) a += (double)e.r2 * (double)R2[(size_t)p * e.ldR2 + oc];
        y[(size_t)p * d.ldY + oc] = (float)a;
      }
    return SRK_OK;
  }
  SRK_REQUIRE(dy, "%s: null pointer", who);
  SRK_REQUIRE(y || d.act == SRK_ACT_NONE, "%s: an activation needs the saved output", who);
  if (int rc = dense_check_ld(who, "ldDy", d.ldDy, d.Cout)) return rc;
  if (d.act != SRK_ACT_NONE)
    if (int rc = dense_check_ld(who, "ldY", d.ldY, d.Cout)) return rc;
  if (direction == 1) {
    SRK_REQUIRE(W && (dA || dB), "%s: null pointer", who);
    SRK_REQUIRE(!add || dA, "%s: add goes into dA, which is null", who);
    if (d.CB == 0) dB = nullptr;
    if (int rc = dense_check_beta(who, betaA)) return rc;
    if (int rc = dense_check_beta(who, betaB)) return rc;
    if (dA)
      if (int rc = dense_check_ld(who, "ldDA", d.ldDA, d.CA)) return rc;
    if (dB)
      if (int rc = dense_check_ld(who, "ldDB", d.ldDB, d.CB)) return rc;
    if (add)
      if (int rc = dense_check_ld(who, "ldAdd", d.ldAdd, d.CA)) return rc;
    std::vector<double> g((size_t)KK * d.Cout);
    for (int64_t p = 0; p < P; ++p) {
      for (int tap = 0; tap < KK; ++tap) {
        const int64_t pp = neighbour(p, pad - tap / K, pad - tap % K);
        for (int oc = 0; oc < d.Cout; ++oc) g[(size_t)tap * d.Cout + oc] = pp < 0 ? 0.0 : grad(pp, oc);
      }
      for (int c = 0; c < Ctot; ++c) {
        const bool inA = c < d.CA;
        float* out = inA ? (dA ? dA + (size_t)p * d.ldDA + c : nullptr) : (dB ? dB + (size_t)p * d.ldDB + (c - d.CA) : nullptr);
        if (!out) continue;
        double a = 0.0;
        for (int tap = 0; tap < KK; ++tap)
          for (int oc = 0; oc < d.Cout; ++oc)
            a += g[(size_t)tap * d.Cout + oc] * (double)W[((size_t)oc * Ctot + c) * KK + tap];
        if (inA && add) a += (double)e.a1 * (double)add[(size_t)p * d.ldAdd + c];
        if ((inA ? betaA : betaB) != 0.f) a += (double)*out;
        *out = (float)a;
      }
    }
    return SRK_OK;
  }
  SRK_REQUIRE(A && (dW || db) && (B || d.CB == 0), "%s: null pointer", who);
  if (int rc = dense_check_beta(who, beta)) return rc;
  if (int rc = dense_check_ld(who, "ldA", d.ldA, d.CA)) return rc;
  if (d.CB)
    if (int rc = dense_check_ld(who, "ldB", d.ldB, d.CB)) return rc;
  std::vector<double> aw(dW ? (size_t)d.Cout * Ctot * KK : 0, 0.0), ab(db ? (size_t)d.Cout : 0, 0.0);
  for (int64_t p = 0; p < P; ++p)
    for (int oc = 0; oc < d.Cout; ++oc) {
      const double g = grad(p, oc);
      if (db) ab[oc] += g;
      if (!dW || g == 0.0) continue;
      for (int tap = 0; tap < KK; ++tap) {
        const int64_t pp = neighbour(p, tap / K - pad, tap % K - pad);
        if (pp < 0) continue;
        for (int c = 0; c < Ctot; ++c) aw[((size_t)oc * Ctot + c) * KK + tap] += g * (double)src(pp, c);
      }
    }
  for (size_t i = 0; i < aw.size(); ++i) dW[i] = (float)(beta != 0.f ? (double)dW[i] + aw[i] : aw[i]);
  for (size_t i = 0; i < ab.size(); ++i) db[i] = (float)(beta != 0.f ? (double)db[i] + ab[i] : ab[i]);
  return SRK_OK;
}

extern "C" int srk_dense_conv_host(const srk_dense_desc* d, int direction, const float* A, const float* B, const float* W,
                                   const float* bias, const float* residual, float* y, const float* dy, const float* add,
                                   float* dA, float betaA, float* dB, float betaB, float* dW, float* db, float beta) {
  return dense_host("dense_conv_host", d, direction, A, B, W, bias, residual, nullptr, nullptr, y, dy, add, dA, betaA, dB,
                    betaB, dW, db, beta);
}

extern "C" int srk_dense_conv_host_ex(const srk_dense_desc* d, int direction, const float* A, const float* B, const float* W,
                                      const float* bias, const float* R1, const float* R2, const srk_dense_epilogue* e, float* y,
                                      const float* dy, const float* add, float* dA, float betaA, float* dB, float betaB,
                                      float* dW, float* db, float beta) {
  return dense_host("dense_conv_host_ex", d, direction, A, B, W, bias, R1, R2, e, y, dy, add, dA, betaA, dB, betaB, dW, db,
                    beta);
}
