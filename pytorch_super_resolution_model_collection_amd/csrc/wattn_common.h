// Shifted-window self-attention (SwinIR): the index arithmetic -- cyclic shift, window partition, relative position
// index, region ids of the shift mask -- and the per-window definition as a plain loop, shared by the kernels
// (csrc/wattn.hip) and the host twin (srk_window_attention_host).  Definition: include/srk.h, DESIGN.md 29.
// No HIP header is needed to read this file: it compiles as plain C++ for the host tools.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRK_WA_HD __host__ __device__ __forceinline__
#else
#define SRK_WA_HD inline
#endif

namespace srk {

constexpr int kWaMaxWindow = 8;    // one lane per token: window^2 <= 64
constexpr int kWaMinWindow = 2;
constexpr int kWaMaxHeadDim = 32;  // q_i, dO_i and one accumulator row live in registers
constexpr float kWaMasked = -100.0f;   // upstream's finite mask value

struct WaGeom {
  int N, H, W, C, heads, d, window, shift;
  int wins_y, wins_x;   // windows along each axis
  int T;                // tokens per window
  int bins;             // (2 * window - 1)^2 rows of the bias table
};

SRK_WA_HD WaGeom wa_geom(int N, int H, int W, int C, int heads, int window, int shift) {
  WaGeom g;
  g.N = N, g.H = H, g.W = W, g.C = C, g.heads = heads, g.d = C / heads, g.window = window, g.shift = shift;
  g.wins_y = H / window, g.wins_x = W / window;
  g.T = window * window;
  g.bins = (2 * window - 1) * (2 * window - 1);
  return g;
}

// Token t of window (wy, wx) sits at (r, c) of the SHIFTED map ...
SRK_WA_HD void wa_shifted_coord(const WaGeom& g, int wy, int wx, int t, int* r, int* c) {
  *r = wy * g.window + t / g.window;
  *c = wx * g.window + t % g.window;
}
// ... which is pixel ((r + shift) mod H, (c + shift) mod W) of the map itself (torch.roll by -shift); the result is
// rolled back by +shift, so the token is read and written at the same pixel.
SRK_WA_HD int wa_unshift(int r, int shift, int extent) {
  const int y = r + shift;
  return y >= extent ? y - extent : y;
}
// pixel index (y * W + x) of token t of window (wy, wx)
SRK_WA_HD int64_t wa_token_pixel(const WaGeom& g, int wy, int wx, int t) {
  int r, c;
  wa_shifted_coord(g, wy, wx, t, &r, &c);
  return (int64_t)wa_unshift(r, g.shift, g.H) * g.W + wa_unshift(c, g.shift, g.W);
}

// rel(i, j) = (y_i - y_j + window - 1) * (2 * window - 1) + (x_i - x_j + window - 1): the bias table's row
SRK_WA_HD int wa_rel_index(int ti, int tj, int window) {
  const int dy = ti / window - tj / window + window - 1, dx = ti % window - tj % window + window - 1;
  return dy * (2 * window - 1) + dx;
}

// band(r, H): 0 if r < H - window, 1 if r < H - shift, else 2 (the three slices of upstream's mask image)
SRK_WA_HD int wa_band(int r, int extent, int window, int shift) {
  return r < extent - window ? 0 : (r < extent - shift ? 1 : 2);
}
// region id of the token at shifted coordinates (r, c); tokens of different regions do not attend to each other
SRK_WA_HD int wa_region(const WaGeom& g, int r, int c) {
  return 3 * wa_band(r, g.H, g.window, g.shift) + wa_band(c, g.W, g.window, g.shift);
}
SRK_WA_HD int wa_token_region(const WaGeom& g, int wy, int wx, int t) {
  if (g.shift == 0) return 0;
  int r, c;
  wa_shifted_coord(g, wy, wx, t, &r, &c);
  return wa_region(g, r, c);
}

// One window and head, as the definition reads: S = d^-0.5 Q K^T + table[rel] + mask, P = softmax_j S, O = P V, and from
// dO: dV = P^T dO, dP = dO V^T, dS = P (dP - rowsum(P dP)), dQ = d^-0.5 dS K, dK = d^-0.5 dS^T Q, dtable[rel] += dS.
// Everything in double.  qkv / out / dout / dqkv are whole tensors ([N][H][W][3C] and [N][H][W][C]); dtable [bins][heads]
// is added to.  dout == nullptr: forward only.
template <typename Real>
inline void wa_window_reference(const WaGeom& g, const float* qkv, const float* table, int n, int wy, int wx, int h,
                                Real* out, const float* dout, Real* dqkv, Real* dtable) {
  const int T = g.T, d = g.d, C = g.C;
  const double scale = 1.0 / sqrt((double)d);
  double P[64 * 64];
  const float* rows[64];
  int64_t pix[64];
  int region[64];
  for (int t = 0; t < T; ++t) {
    pix[t] = (int64_t)n * g.H * g.W + wa_token_pixel(g, wy, wx, t);
    rows[t] = qkv + pix[t] * 3 * C + h * d;
    region[t] = wa_token_region(g, wy, wx, t);
  }
  for (int i = 0; i < T; ++i) {
    double mx = -1e300;
    for (int j = 0; j < T; ++j) {
      double s = 0.0;
      for (int c = 0; c < d; ++c) s += (double)rows[i][c] * (double)rows[j][C + c];
      s = s * scale + (double)table[wa_rel_index(i, j, g.window) * g.heads + h];
      if (region[i] != region[j]) s += (double)kWaMasked;
      P[i * 64 + j] = s;
      mx = s > mx ? s : mx;
    }
    double sum = 0.0;
    for (int j = 0; j < T; ++j) sum += (P[i * 64 + j] = exp(P[i * 64 + j] - mx));
    for (int j = 0; j < T; ++j) P[i * 64 + j] /= sum;
    for (int c = 0; c < d; ++c) {
      double o = 0.0;
      for (int j = 0; j < T; ++j) o += P[i * 64 + j] * (double)rows[j][2 * C + c];
      out[pix[i] * C + h * d + c] = (Real)o;
    }
  }
  if (!dout) return;
  double dS[64 * 64];
  for (int i = 0; i < T; ++i) {
    const float* go = dout + pix[i] * C + h * d;
    double D = 0.0;
    for (int j = 0; j < T; ++j) {
      double dp = 0.0;
      for (int c = 0; c < d; ++c) dp += (double)go[c] * (double)rows[j][2 * C + c];
      dS[i * 64 + j] = dp;
      D += P[i * 64 + j] * dp;
    }
    for (int j = 0; j < T; ++j) {
      dS[i * 64 + j] = P[i * 64 + j] * (dS[i * 64 + j] - D);
      dtable[wa_rel_index(i, j, g.window) * g.heads + h] += (Real)dS[i * 64 + j];
    }
  }
  for (int i = 0; i < T; ++i)
    for (int c = 0; c < d; ++c) {
      double dq = 0.0, dk = 0.0, dv = 0.0;
      for (int j = 0; j < T; ++j) {
        dq += dS[i * 64 + j] * (double)rows[j][C + c];
        dk += dS[j * 64 + i] * (double)rows[j][c];
        dv += P[j * 64 + i] * (double)dout[pix[j] * C + h * d + c];
      }
      Real* gr = dqkv + pix[i] * 3 * C + h * d + c;
      gr[0] = (Real)(dq * scale), gr[C] = (Real)(dk * scale), gr[2 * C] = (Real)dv;
    }
}

}  // namespace srk
