// Spectral normalisation of convolution filters (torch.nn.utils.spectral_norm, one power iteration, dim = 0) for a whole
// discriminator at once.  Definition: include/srk.h and DESIGN.md 31; the per-element formulas: spectral_norm_common.h,
// shared with the host twin below.  W is the [R][K] view of a filter, R = out channels, K = in * kh * kw.
//
// Forward, three launches for up to SRK_SPECTRAL_MAX_LAYERS layers (blockIdx -> (layer, tile) through a table passed by
// value; the reductions depend on each other across blocks, hence three):
//   k_sn_wtu     t = W^T u: a block owns 16 V columns and all rows; 16 row groups add their rows in index order and meet in
//                LDS in index order.  Training mode only.
//   k_sn_wv      every block finishes ||t|| and v = t / max(||t||, eps) in LDS -- eval mode: reads the stored v instead --
//                then s = W v for its 8 rows, a wave a row.
//   k_sn_apply   every block finishes ||s||, u = s / max(||s||, eps) and sigma = u . s from the R doubles of s -- eval mode:
//                sigma = stored u . s -- and writes its tile of w_sn = W / sigma.  The layer's first block also writes u
//                and the node's copy of (u, v, sigma).
// Backward, two launches per layer: k_sn_dot (per-block partials of <G, w_sn>) and k_sn_grad (finishes them, writes dW).
// Every sum is double in an order that is a function of the shape alone; no atomics; u, v and w_sn are stored fp32 and read
// back as stored.  16-byte accesses along K where K % 4 == 0 and the pointers allow, 4-byte accesses otherwise.
#include "spectral_norm_common.h"
#include "srk_common.h"

namespace srk {

constexpr int kSnRowsB = 8;       // rows of W one k_sn_wv block multiplies
constexpr int kSnTile = 4096;     // elements of W one k_sn_apply / k_sn_dot / k_sn_grad block handles
constexpr int kSnMaxK = 16384;    // k_sn_wv keeps t in LDS as doubles: 128 KB

struct SnLayer {
  const float* W;
  float *u, *v, *w_sn, *saved;
  double* P;                      // [K] t = W^T u
  double* s;                      // [R] W v
  int R, K, vec;
  int a0, b0, c0;                 // the layer's first block in the three grids
};
struct SnTable {
  SnLayer L[SRK_SPECTRAL_MAX_LAYERS];
  int n;
};

__device__ __forceinline__ int sn_layer_of(const SnTable& t, int bx, int which) {
  int l = t.n - 1;
  for (; l > 0; --l) {
    const int first = which == 0 ? t.L[l].a0 : (which == 1 ? t.L[l].b0 : t.L[l].c0);
    if (bx >= first) break;
  }
  return l;
}

template <int V>
__device__ __forceinline__ void sn_wtu_tile(const SnLayer& L, int local, double* sh) {
  // 16 column groups of V columns x 16 row groups: a thread adds its rows r = rg, rg + 16, ... in that order, the row groups
  // meet in LDS and are added in index order: t is complete, no partials leave the block
  const int cg = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int k = (local * 16 + cg) * V;
  double acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.0;
  if (k < L.K) {                  // (K % V == 0 on this path: k < K means k + V <= K)
#pragma unroll 4
    for (int r = rg; r < L.R; r += 16) {
      const double ur = (double)L.u[r];
      const typename Vec<V>::T w = Vec<V>::load(L.W + (size_t)r * L.K, (size_t)k / V);
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] += (double)Vec<V>::at(w, i) * ur;
    }
  }
#pragma unroll
  for (int i = 0; i < V; ++i) sh[(rg * 16 + cg) * V + i] = acc[i];
  __syncthreads();
  if (rg == 0 && k < L.K) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
      double t = 0.0;
      for (int g = 0; g < 16; ++g) t += sh[(g * 16 + cg) * V + i];
      L.P[k + i] = t;
    }
  }
}

__global__ __launch_bounds__(256) void k_sn_wtu(const SnTable t) {
  const int l = sn_layer_of(t, blockIdx.x, 0);
  const SnLayer& L = t.L[l];
  __shared__ double sh[256 * 4];
  const int local = (int)blockIdx.x - L.a0;
  if (L.vec)
    sn_wtu_tile<4>(L, local, sh);
  else
    sn_wtu_tile<1>(L, local, sh);
}

template <int V>
__device__ __forceinline__ double sn_row_dot(const float* __restrict__ row, const double* __restrict__ sh, int K, int lane) {
  double acc = 0.0;
#pragma unroll 4
  for (int k = lane * V; k < K; k += 64 * V) {
    const typename Vec<V>::T w = Vec<V>::load(row, (size_t)k / V);
#pragma unroll
    for (int i = 0; i < V; ++i) acc += (double)Vec<V>::at(w, i) * sh[k + i];
  }
  return wave_sum_d(acc);
}

__global__ __launch_bounds__(256) void k_sn_wv(const SnTable t, int training, double eps) {
  extern __shared__ double sn_sh[];                 // [K of this layer] t, then v as stored; 4 doubles behind the largest K
  __shared__ double sm[4];
  const int l = sn_layer_of(t, blockIdx.x, 1);
  const SnLayer& L = t.L[l];
  const int local = (int)blockIdx.x - L.b0, K = L.K;
  const int tid = threadIdx.x;
  if (training) {
    double sq = 0.0;
    for (int k = tid; k < K; k += 256) {
      const double tk = L.P[k];
      sn_sh[k] = tk;
      sq += tk * tk;
    }
    const double nt = sn_norm(block_sum_256_d(sq, sm));
    for (int k = tid; k < K; k += 256) {            // (each thread rewrites the elements it wrote itself)
      const float vk = (float)sn_normalized(sn_sh[k], nt, eps);
      sn_sh[k] = (double)vk;
      if (local == 0) L.v[k] = vk;
    }
  } else {
    for (int k = tid; k < K; k += 256) sn_sh[k] = (double)L.v[k];
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  const int r0 = local * kSnRowsB, r1 = min(L.R, r0 + kSnRowsB);
  for (int r = r0 + wave; r < r1; r += 4) {
    const float* row = L.W + (size_t)r * K;
    const double d = L.vec ? sn_row_dot<4>(row, sn_sh, K, lane) : sn_row_dot<1>(row, sn_sh, K, lane);
    if (lane == 0) L.s[r] = d;
  }
}

template <int V>
__device__ __forceinline__ void sn_apply_tile(const SnLayer& L, int local, double sigma) {
  const size_t total = (size_t)L.R * L.K, base = (size_t)local * kSnTile;
  const size_t end = base + kSnTile < total ? base + kSnTile : total;
  for (size_t i = base + (size_t)threadIdx.x * V; i < end; i += 256 * V) {   // (total % V == 0 on this path)
    const typename Vec<V>::T w = Vec<V>::load(L.W, i / V);
    typename Vec<V>::T o;
#pragma unroll
    for (int e = 0; e < V; ++e) Vec<V>::set(o, e, (float)sn_weight((double)Vec<V>::at(w, e), sigma));
    Vec<V>::store(L.w_sn, i / V, o);
  }
}

__global__ __launch_bounds__(256) void k_sn_apply(const SnTable t, int training, double eps) {
  __shared__ double sm[4];
  const int l = sn_layer_of(t, blockIdx.x, 2);
  const SnLayer& L = t.L[l];
  const int local = (int)blockIdx.x - L.c0, R = L.R, tid = threadIdx.x;
  double ns = 0.0;
  if (training) {
    double sq = 0.0;
    for (int r = tid; r < R; r += 256) sq += L.s[r] * L.s[r];
    ns = sn_norm(block_sum_256_d(sq, sm));
  }
  double acc = 0.0;
  for (int r = tid; r < R; r += 256) {
    const float ur = training ? (float)sn_normalized(L.s[r], ns, eps) : L.u[r];
    acc += (double)ur * L.s[r];
  }
  const double sigma = block_sum_256_d(acc, sm);
  if (L.vec)
    sn_apply_tile<4>(L, local, sigma);
  else
    sn_apply_tile<1>(L, local, sigma);
  if (local != 0) return;
  // the layer's first block: u in place, and the copies the backward of THIS forward reads (nobody reads u or v in this
  // launch in training mode: the other blocks work from s)
  for (int r = tid; r < R; r += 256) {
    const float ur = training ? (float)sn_normalized(L.s[r], ns, eps) : L.u[r];
    if (training) L.u[r] = ur;
    if (L.saved) L.saved[r] = ur;
  }
  if (L.saved) {
    for (int k = tid; k < L.K; k += 256) L.saved[R + k] = L.v[k];
    if (tid == 0) L.saved[R + L.K] = (float)sigma;
  }
}

template <int V>
__global__ __launch_bounds__(256) void k_sn_dot(const float* __restrict__ G, const float* __restrict__ w_sn, size_t total,
                                                double* __restrict__ part) {
  __shared__ double sm[4];
  const size_t base = (size_t)blockIdx.x * kSnTile;
  const size_t end = base + kSnTile < total ? base + kSnTile : total;
  double acc = 0.0;
  for (size_t i = base + (size_t)threadIdx.x * V; i < end; i += 256 * V) {
    const typename Vec<V>::T g = Vec<V>::load(G, i / V), w = Vec<V>::load(w_sn, i / V);
#pragma unroll
    for (int e = 0; e < V; ++e) acc += (double)Vec<V>::at(g, e) * (double)Vec<V>::at(w, e);
  }
  store_block_sum_256_d(acc, sm, part + blockIdx.x);
}

template <int V>
__global__ __launch_bounds__(256) void k_sn_grad(const float* __restrict__ G, const float* __restrict__ saved, int R, int K,
                                                 const double* __restrict__ part, int nparts, float* __restrict__ dW,
                                                 float beta) {
  __shared__ double sm[4];
  const double dot = sum_partials_256_d(part, nparts, sm);
  const double sigma = (double)saved[R + K];
  const size_t total = (size_t)R * K, base = (size_t)blockIdx.x * kSnTile;
  const size_t end = base + kSnTile < total ? base + kSnTile : total;
  for (size_t i = base + (size_t)threadIdx.x * V; i < end; i += 256 * V) {
    const int r = (int)(i / (size_t)K), k = (int)(i - (size_t)r * K);      // (K % V == 0: the V elements share the row)
    const double ur = (double)saved[r];
    const typename Vec<V>::T g = Vec<V>::load(G, i / V);
    typename Vec<V>::T o;
    if (beta != 0.f) o = Vec<V>::load(dW, i / V);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const double d = sn_grad((double)Vec<V>::at(g, e), dot, ur, (double)saved[R + k + e], sigma);
      Vec<V>::set(o, e, beta != 0.f ? beta * Vec<V>::at(o, e) + (float)d : (float)d);
    }
    Vec<V>::store(dW, i / V, o);
  }
}

static int sn_check_layers(const char* who, const srk_spectral_layer* layers, int n) {
  SRK_REQUIRE(layers != nullptr, "%s: null layer table", who);
  SRK_REQUIRE(n >= 1 && n <= SRK_SPECTRAL_MAX_LAYERS, "%s: %d layers, 1 .. %d are taken", who, n, SRK_SPECTRAL_MAX_LAYERS);
  for (int l = 0; l < n; ++l) {
    const srk_spectral_layer& a = layers[l];
    SRK_REQUIRE(a.W && a.u && a.v && a.w_sn, "%s: layer %d: null pointer", who, l);
    SRK_REQUIRE(a.R >= 1 && a.K >= 1, "%s: layer %d: R = %d, K = %d", who, l, a.R, a.K);
    SRK_REQUIRE(a.K <= kSnMaxK, "%s: layer %d: K = %d, at most %d columns are taken", who, l, a.K, kSnMaxK);
    SRK_REQUIRE((size_t)a.R * a.K < ((size_t)1 << 31), "%s: layer %d: %d x %d elements", who, l, a.R, a.K);
  }
  return SRK_OK;
}

static size_t sn_layer_ws(int R, int K) { return ((size_t)K + (size_t)R) * sizeof(double); }

}  // namespace srk

using namespace srk;

extern "C" size_t srk_spectral_norm_workspace(const srk_spectral_layer* layers, int n) {
  if (sn_check_layers("spectral_norm_workspace", layers, n) != SRK_OK) return 0;
  size_t bytes = 0;
  for (int l = 0; l < n; ++l) bytes += sn_layer_ws(layers[l].R, layers[l].K);
  return bytes;
}

extern "C" int srk_spectral_norm_forward(const srk_spectral_layer* layers, int n, int training, double eps, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  const char* who = "spectral_norm_forward";
  const int rc = sn_check_layers(who, layers, n);
  if (rc != SRK_OK) return rc;
  SRK_REQUIRE(eps >= 0.0, "%s: eps = %g", who, eps);
  const size_t need = srk_spectral_norm_workspace(layers, n);
  SRK_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %zu bytes, %zu are needed", who, workspace_bytes, need);
  SRK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: workspace is not 8-byte aligned", who);
  SnTable t;
  t.n = n;
  double* ws = reinterpret_cast<double*>(workspace);
  int a = 0, b = 0, c = 0, maxK = 0;
  for (int l = 0; l < n; ++l) {
    const srk_spectral_layer& in = layers[l];
    SnLayer& L = t.L[l];
    L.W = in.W, L.u = in.u, L.v = in.v, L.w_sn = in.w_sn, L.saved = in.saved;
    L.R = in.R, L.K = in.K;
    L.vec = (L.K % 4 == 0 && aligned16(L.W, L.w_sn)) ? 1 : 0;
    L.P = ws;
    L.s = ws + L.K;
    ws += (size_t)L.K + L.R;
    L.a0 = a, L.b0 = b, L.c0 = c;
    a += (int)cdiv((size_t)L.K, (size_t)16 * (L.vec ? 4 : 1));
    b += (int)cdiv((size_t)L.R, (size_t)kSnRowsB);
    c += (int)cdiv((size_t)L.R * L.K, (size_t)kSnTile);
    maxK = L.K > maxK ? L.K : maxK;
  }
  hipStream_t s = (hipStream_t)stream;
  if (training) hipLaunchKernelGGL(k_sn_wtu, dim3(a), dim3(256), 0, s, t);
  launch_lds<k_sn_wv>(dim3(b), dim3(256), (size_t)maxK * sizeof(double), s, t, training ? 1 : 0, eps);
  hipLaunchKernelGGL(k_sn_apply, dim3(c), dim3(256), 0, s, t, training ? 1 : 0, eps);
  return check_launch(who);
}

extern "C" size_t srk_spectral_norm_backward_workspace(int R, int K) {
  if (R < 1 || K < 1) return 0;
  return (size_t)cdiv((size_t)R * K, (size_t)kSnTile) * sizeof(double);
}

extern "C" int srk_spectral_norm_backward(const float* G, const float* w_sn, const float* saved, int R, int K, float* dW,
                                          float beta, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "spectral_norm_backward";
  SRK_REQUIRE(G && w_sn && saved && dW, "%s: null pointer", who);
  SRK_REQUIRE(R >= 1 && K >= 1, "%s: R = %d, K = %d", who, R, K);
  SRK_REQUIRE((size_t)R * K < ((size_t)1 << 31), "%s: %d x %d elements", who, R, K);
  const size_t need = srk_spectral_norm_backward_workspace(R, K);
  SRK_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %zu bytes, %zu are needed", who, workspace_bytes, need);
  SRK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: workspace is not 8-byte aligned", who);
  const size_t total = (size_t)R * K;
  const int nb = (int)cdiv(total, (size_t)kSnTile);
  double* part = reinterpret_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  if (K % 4 == 0 && aligned16(G, w_sn, dW)) {
    hipLaunchKernelGGL(k_sn_dot<4>, dim3(nb), dim3(256), 0, s, G, w_sn, total, part);
    hipLaunchKernelGGL(k_sn_grad<4>, dim3(nb), dim3(256), 0, s, G, saved, R, K, (const double*)part, nb, dW, beta);
  } else {
    hipLaunchKernelGGL(k_sn_dot<1>, dim3(nb), dim3(256), 0, s, G, w_sn, total, part);
    hipLaunchKernelGGL(k_sn_grad<1>, dim3(nb), dim3(256), 0, s, G, saved, R, K, (const double*)part, nb, dW, beta);
  }
  return check_launch(who);
}

extern "C" int srk_spectral_norm_host(const float* W, int R, int K, int training, double eps, double* u, double* v,
                                      double* w_sn, double* sigma_out, const double* G, double* dW) {
  const char* who = "spectral_norm_host";
  SRK_REQUIRE(W && u && v && w_sn && sigma_out, "%s: null pointer", who);
  SRK_REQUIRE((G == nullptr) == (dW == nullptr), "%s: G and dW come together", who);
  SRK_REQUIRE(R >= 1 && K >= 1, "%s: R = %d, K = %d", who, R, K);
  SRK_REQUIRE(eps >= 0.0, "%s: eps = %g", who, eps);
  if (training) {
    double sq = 0.0;
    for (int k = 0; k < K; ++k) {
      double t = 0.0;
      for (int r = 0; r < R; ++r) t += (double)W[(size_t)r * K + k] * u[r];
      w_sn[k] = t;                 // (w_sn holds R * K >= K doubles: scratch until it is written below)
      sq += t * t;
    }
    const double nt = sn_norm(sq);
    for (int k = 0; k < K; ++k) v[k] = sn_normalized(w_sn[k], nt, eps);
  }
  double ns = 0.0, sigma = 0.0;      // (s = W v is computed twice in training mode: no scratch row to keep it in)
  if (training) {
    double sq = 0.0;
    for (int r = 0; r < R; ++r) {
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += (double)W[(size_t)r * K + k] * v[k];
      sq += s * s;
    }
    ns = sn_norm(sq);
  }
  for (int r = 0; r < R; ++r) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += (double)W[(size_t)r * K + k] * v[k];
    if (training) u[r] = sn_normalized(s, ns, eps);
    sigma += u[r] * s;
  }
  *sigma_out = sigma;
  const size_t total = (size_t)R * K;
  for (size_t i = 0; i < total; ++i) w_sn[i] = sn_weight((double)W[i], sigma);
  if (G) {
    double dot = 0.0;
    for (size_t i = 0; i < total; ++i) dot += G[i] * w_sn[i];
    for (int r = 0; r < R; ++r)
      for (int k = 0; k < K; ++k) dW[(size_t)r * K + k] = sn_grad(G[(size_t)r * K + k], dot, u[r], v[k], sigma);
  }
  return SRK_OK;
}
