// The classical degradation model of blind super-resolution on the loader's 8-bit patches, LR = (HR * k) shrunk + n:
// a per-patch anisotropic Gaussian blur in front of the Pillow-exact shrink (k_blur_u8) and additive Gaussian noise behind
// it (k_noise_u8).  Both are defined to the bit (include/srk.h): fp64 sums in a fixed tap order, Philox4x32-10
// and Box-Muller in fp64, so a numpy restatement gives the same bytes.
//
// k_blur_u8<K>: a block owns kBlurTH x kBlurTW outputs of one plane, stages them plus the halo of K/2 (reflect-101 at the
// plane's borders) as bytes in LDS and the patch's K x K fp64 table beside them, and every thread makes a horizontal run of
// kBlurRun outputs: per tap row it reads K + kBlurRun - 1 staged bytes as whole dwords, converts each to fp64 ONCE and uses
// it in up to kBlurRun sums.  Taps are added in row-major (i, j) order.
// k_noise_u8: a thread makes the four normals of one Philox counter and the four consecutive elements that take them.
#include "srk_common.h"
#include "degrade_common.h"

namespace srk {

constexpr int kBlurTH = 16, kBlurTW = 64, kBlurRun = 4;
static_assert(kBlurTH * kBlurTW == 256 * kBlurRun && kBlurTW % kBlurRun == 0 && kBlurRun == 4,
              "256 threads, a run of four outputs (one dword of bytes) each");

// Reflect-101 of a coordinate first clamped to [-r, n - 1 + r] (n > r): what lies further out belongs to outputs past the
// plane's edge, which are never stored, and must only stay inside the plane.
__device__ __forceinline__ int blur_reflect(int c, int n, int r) {
  c = c < -r ? -r : (c > n - 1 + r ? n - 1 + r : c);
  return c < 0 ? -c : (c >= n ? 2 * (n - 1) - c : c);
}

template <int K>
__global__ __launch_bounds__(256) void k_blur_u8(const uint8_t* __restrict__ x, uint8_t* __restrict__ y,
                                                 const double* __restrict__ w, int planes_per_patch, int H, int W,
                                                 int tiles_x, int tiles_per_plane) {
  constexpr int R = K / 2;
  constexpr int NW = (K + kBlurRun - 1 + 3) / 4;      // dwords of staged bytes a thread reads per tap row
  constexpr int PITCH = kBlurTW - kBlurRun + 4 * NW;  // bytes per staged row: the last thread's NW dwords end here
  constexpr int SH = kBlurTH + K - 1;
  static_assert(PITCH % 4 == 0 && PITCH >= kBlurTW + K - 1, "rows start on a dword and hold the tile with its halo");
  __shared__ double sw[K * K];
  __shared__ uint32_t spx[SH * PITCH / 4];

  const int plane = blockIdx.x / tiles_per_plane, t = blockIdx.x - plane * tiles_per_plane;
  const int ty0 = (t / tiles_x) * kBlurTH, tx0 = (t % tiles_x) * kBlurTW;
  const uint8_t* __restrict__ xp = x + (size_t)plane * H * W;
  const double* __restrict__ wp = w + (size_t)(plane / planes_per_patch) * (K * K);
  for (int i = threadIdx.x; i < K * K; i += 256) sw[i] = wp[i];
  uint8_t* sb = reinterpret_cast<uint8_t*>(spx);
  for (int i = threadIdx.x; i < SH * PITCH; i += 256) {
    const int r = i / PITCH, c = i - r * PITCH;
    sb[i] = xp[(size_t)blur_reflect(ty0 + r - R, H, R) * W + blur_reflect(tx0 + c - R, W, R)];
  }
  __syncthreads();

  const int row = threadIdx.x / (kBlurTW / kBlurRun), cx = (threadIdx.x % (kBlurTW / kBlurRun)) * kBlurRun;
  double acc[kBlurRun] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int i = 0; i < K; ++i) {
    const uint32_t* rp = spx + ((row + i) * PITCH + cx) / 4;
    double p[4 * NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const uint32_t v = rp[k];
      p[4 * k] = (double)(v & 255u);
      p[4 * k + 1] = (double)((v >> 8) & 255u);
      p[4 * k + 2] = (double)((v >> 16) & 255u);
      p[4 * k + 3] = (double)(v >> 24);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double wv = sw[i * K + j];
#pragma unroll
      for (int o = 0; o < kBlurRun; ++o) acc[o] += wv * p[j + o];
    }
  }

  const int oy = ty0 + row, ox = tx0 + cx;
  if (oy >= H || ox >= W) return;
  uint8_t q[kBlurRun];
#pragma unroll
  for (int o = 0; o < kBlurRun; ++o) q[o] = (uint8_t)(int)floor(fmin(fmax(acc[o], 0.0), 255.0) + 0.5);
  uint8_t* yp = y + (size_t)plane * H * W + (size_t)oy * W + ox;
  if (ox + kBlurRun <= W && (reinterpret_cast<uintptr_t>(yp) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(yp) = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
  } else {
#pragma unroll
    for (int o = 0; o < kBlurRun; ++o)
      if (ox + o < W) yp[o] = q[o];
  }
}

template <int K>
static void launch_blur(const uint8_t* x, uint8_t* y, const double* w, int planes_per_patch, int H, int W, int tiles_x,
                        int tiles_per_plane, unsigned blocks, hipStream_t s) {
  hipLaunchKernelGGL(k_blur_u8<K>, dim3(blocks), dim3(256), 0, s, x, y, w, planes_per_patch, H, W, tiles_x, tiles_per_plane);
}

// y[e] = float(clamp(round_half_up(x[e] + sigma[patch of e] * z[e]), 0, 255)) / 255.0f over `total` elements; with
// OutT = uint8_t the clamped level itself (srk_noise_u8_bytes: what the JPEG stage takes).
template <typename OutT>
__global__ __launch_bounds__(256) void k_noise_u8(const uint8_t* __restrict__ x, OutT* __restrict__ y,
                                                  const double* __restrict__ sigma, uint64_t seed, int64_t elems_per_patch,
                                                  int64_t total) {
  const int64_t groups = (total + 3) >> 2;
  constexpr bool kBytes = std::is_same<OutT, uint8_t>::value;
  const bool vec = (kBytes ? (reinterpret_cast<uintptr_t>(y) & 3) == 0 : aligned16(y)) && (reinterpret_cast<uintptr_t>(x) & 3) == 0;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < groups; q += (int64_t)gridDim.x * 256) {
    const int64_t e0 = q << 2;
    const int n = total - e0 < 4 ? (int)(total - e0) : 4;
    uint8_t in[4] = {0, 0, 0, 0};
    double sg[4] = {0.0, 0.0, 0.0, 0.0};
    if (vec && n == 4) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(x + e0);
      in[0] = (uint8_t)v, in[1] = (uint8_t)(v >> 8), in[2] = (uint8_t)(v >> 16), in[3] = (uint8_t)(v >> 24);
    } else {
      for (int k = 0; k < n; ++k) in[k] = x[e0 + k];
    }
    bool any = false;
    for (int k = 0; k < n; ++k) {
      sg[k] = sigma[(e0 + k) / elems_per_patch];
      any = any || sg[k] != 0.0;
    }
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    if (any) noise_normals4(seed, (uint64_t)q, z);   // (a group whose sigmas are all zero adds 0 * z: skip the generator)
    OutT out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double r = floor((double)in[k] + sg[k] * z[k] + 0.5);
      if constexpr (kBytes) out[k] = (uint8_t)(int)fmin(fmax(r, 0.0), 255.0);
      else out[k] = (float)fmin(fmax(r, 0.0), 255.0) / 255.f;
    }
    if (vec && n == 4) {
      if constexpr (kBytes) {
        *reinterpret_cast<uint32_t*>(y + e0) =
            (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16) | ((uint32_t)out[3] << 24);
      } else {
        f32x4 o = {out[0], out[1], out[2], out[3]};
        *reinterpret_cast<f32x4*>(y + e0) = o;
      }
    } else {
      for (int k = 0; k < n; ++k) y[e0 + k] = out[k];
    }
  }
}

// srk_noise2_u8: a thread makes up to four consecutive elements through noise2_group (degrade_common.h), the body the host
// twin loops over.  Bytes are read and written one by one: the per-patch mode decides what an element needs.
__global__ __launch_bounds__(256) void k_noise2_u8(const uint8_t* __restrict__ x, uint8_t* __restrict__ y,
                                                   const double* __restrict__ mode, const double* __restrict__ gray,
                                                   const double* __restrict__ amount, const double* __restrict__ cdf,
                                                   uint64_t seed, uint32_t stage, int C, int64_t HW, int color, int64_t total) {
  const int64_t groups = (total + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < groups; q += (int64_t)gridDim.x * 256) {
    const int64_t e0 = q << 2;
    noise2_group(x, y, mode, gray, amount, cdf, seed, stage, C, HW, color, e0, total - e0 < 4 ? (int)(total - e0) : 4);
  }
}

}  // namespace srk

using namespace srk;

extern "C" int srk_blur_u8(const uint8_t* x, uint8_t* y, const double* w, int planes_per_patch, int B, int H, int W, int K,
                           void* stream) {
  SRK_REQUIRE(x && y && w, "blur_u8: null pointer");
  SRK_REQUIRE(planes_per_patch > 0 && B > 0 && H > 0 && W > 0, "blur_u8: bad dims (planes per patch %d, B %d, %d x %d)",
              planes_per_patch, B, H, W);
  SRK_REQUIRE(K >= 3 && K <= kBlurMaxK && (K & 1), "blur_u8: K must be odd and in [3, %d] (got %d)", kBlurMaxK, K);
  SRK_REQUIRE(H > K / 2 && W > K / 2, "blur_u8: a %d x %d plane cannot mirror a halo of %d (reflect-101 needs H, W > K / 2)",
              H, W, K / 2);
  const int tiles_x = (W + kBlurTW - 1) / kBlurTW, tiles_y = (H + kBlurTH - 1) / kBlurTH;
  const int64_t blocks = (int64_t)planes_per_patch * B * tiles_x * tiles_y;
  SRK_REQUIRE(blocks <= 0x7fffffff, "blur_u8: %lld tiles are more than one launch takes", (long long)blocks);
  hipStream_t s = (hipStream_t)stream;
  const int tpp = tiles_x * tiles_y;
  switch (K) {
#define SRK_BLUR_CASE(KK) \
  case KK: launch_blur<KK>(x, y, w, planes_per_patch, H, W, tiles_x, tpp, (unsigned)blocks, s); break;
    SRK_BLUR_CASE(3) SRK_BLUR_CASE(5) SRK_BLUR_CASE(7) SRK_BLUR_CASE(9) SRK_BLUR_CASE(11) SRK_BLUR_CASE(13)
    SRK_BLUR_CASE(15) SRK_BLUR_CASE(17) SRK_BLUR_CASE(19) SRK_BLUR_CASE(21)
#undef SRK_BLUR_CASE
  }
  return check_launch("blur_u8");
}

template <typename OutT>
static int launch_noise(const char* what, const uint8_t* x, OutT* y, const double* sigma, uint64_t seed, int B,
                        int64_t elems_per_patch, void* stream) {
  SRK_REQUIRE(x && y && sigma, "%s: null pointer", what);
  SRK_REQUIRE(B > 0 && elems_per_patch > 0, "%s: bad dims (B %d, %lld elements per patch)", what, B,
              (long long)elems_per_patch);
  const int64_t total = (int64_t)B * elems_per_patch;
  hipLaunchKernelGGL(k_noise_u8<OutT>, dim3(grid_for((size_t)((total + 3) >> 2), 256, (size_t)kNumCU * 8)), dim3(256), 0,
                     (hipStream_t)stream, x, y, sigma, seed, elems_per_patch, total);
  return check_launch(what);
}

extern "C" int srk_noise_u8(const uint8_t* x, float* y, const double* sigma, uint64_t seed, int B, int64_t elems_per_patch,
                            void* stream) {
  return launch_noise("noise_u8", x, y, sigma, seed, B, elems_per_patch, stream);
}

extern "C" int srk_noise_u8_bytes(const uint8_t* x, uint8_t* y, const double* sigma, uint64_t seed, int B,
                                  int64_t elems_per_patch, void* stream) {
  return launch_noise("noise_u8_bytes", x, y, sigma, seed, B, elems_per_patch, stream);
}

extern "C" int srk_blur_weights_host(double s1, double s2, double theta, int K, double* w) {
#pragma clang fp contract(off)
  SRK_REQUIRE(w, "blur_weights_host: null pointer");
  SRK_REQUIRE(K >= 1 && K <= kBlurMaxK && (K & 1), "blur_weights_host: K must be odd and in [1, %d] (got %d)", kBlurMaxK, K);
  SRK_REQUIRE(s1 > 0.0 && s2 > 0.0, "blur_weights_host: sigmas must be positive (got %g, %g)", s1, s2);
  const int r = K / 2;
  const double c = cos(theta), s = sin(theta);
  // exp() is the cost of a table (the loader thread makes one per patch): w[i][j] and w[K-1-i][K-1-j] are the same
  // expression of (-x, -y), the same bits, so half the table is computed and mirrored.
  const int n = K * K;
  for (int idx = 0; idx <= n / 2; ++idx) {
    const double xx = (double)(idx % K - r), yy = (double)(idx / K - r);
    const double u = c * xx + s * yy, v = -s * xx + c * yy;
    w[idx] = w[n - 1 - idx] = exp(-0.5 * (u * u / (s1 * s1) + v * v / (s2 * s2)));
  }
  // The sum is compensated (Neumaier): a plain running sum of 441 terms is off by up to ~1.5e-15 of the total, and the
  // normalised table would then sum to 1 only that closely.
  double sum = 0.0, comp = 0.0;
  for (int idx = 0; idx < n; ++idx) {
    const double e = w[idx], t = sum + e;
    comp += fabs(sum) >= fabs(e) ? (sum - t) + e : (e - t) + sum;
    sum = t;
  }
  sum += comp;
  for (int i = 0; i < K * K; ++i) w[i] /= sum;
  return SRK_OK;
}

extern "C" int srk_philox4x32_10_host(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  SRK_REQUIRE(counter && key && out, "philox4x32_10_host: null pointer");
  uint32_t c[4] = {counter[0], counter[1], counter[2], counter[3]};
  philox4x32_10(c, key[0], key[1]);
  for (int i = 0; i < 4; ++i) out[i] = c[i];
  return SRK_OK;
}

extern "C" int srk_noise_normals_host(uint64_t seed, int64_t first_elem, int64_t n, double* z) {
  SRK_REQUIRE(z, "noise_normals_host: null pointer");
  SRK_REQUIRE(first_elem >= 0 && n >= 0, "noise_normals_host: negative range (%lld, %lld)", (long long)first_elem,
              (long long)n);
  double g[4];
  int64_t have = -1;
  for (int64_t k = 0; k < n; ++k) {
    const int64_t e = first_elem + k;
    if ((e >> 2) != have) {
      have = e >> 2;
      noise_normals4(seed, (uint64_t)have, g);
    }
    z[k] = g[e & 3];
  }
  return SRK_OK;
}

// ---- the second-order chain (data.Degradation2) ----------------------------------------------------------
static int noise2_check(const char* what, const void* x, const void* y, const double* mode, const double* gray,
                        const double* amount, const double* cdf, int stage, int B, int C, int H, int W) {
  SRK_REQUIRE(x && y && mode && gray && amount && cdf, "%s: null pointer", what);
  SRK_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad dims (B %d, %d x %d)", what, B, H, W);
  SRK_REQUIRE(C == 1 || C == 3, "%s: C must be 1 or 3 (got %d)", what, C);
  SRK_REQUIRE(stage >= 0 && stage <= 2, "%s: stage must be 0, 1 or 2 (got %d)", what, stage);
  return SRK_OK;
}

extern "C" int srk_noise2_u8(const uint8_t* x, uint8_t* y, const double* mode, const double* gray, const double* amount,
                             const double* cdf, uint64_t seed, int stage, int B, int C, int H, int W, int color,
                             void* stream) {
  if (int rc = noise2_check("noise2_u8", x, y, mode, gray, amount, cdf, stage, B, C, H, W)) return rc;
  const int64_t HW = (int64_t)H * W, total = HW * C * B;
  hipLaunchKernelGGL(k_noise2_u8, dim3(grid_for((size_t)((total + 3) >> 2), 256, (size_t)kNumCU * 8)), dim3(256), 0,
                     (hipStream_t)stream, x, y, mode, gray, amount, cdf, seed, (uint32_t)stage, C, HW, color ? 1 : 0, total);
  return check_launch("noise2_u8");
}

extern "C" int srk_noise2_u8_host(const uint8_t* x, uint8_t* y, const double* mode, const double* gray,
                                  const double* amount, const double* cdf, uint64_t seed, int stage, int B, int C, int H,
                                  int W, int color) {
  if (int rc = noise2_check("noise2_u8_host", x, y, mode, gray, amount, cdf, stage, B, C, H, W)) return rc;
  const int64_t HW = (int64_t)H * W, total = HW * C * B;
  for (int64_t e0 = 0; e0 < total; e0 += 4)
    noise2_group(x, y, mode, gray, amount, cdf, seed, (uint32_t)stage, C, HW, color ? 1 : 0, e0,
                 total - e0 < 4 ? (int)(total - e0) : 4);
  return SRK_OK;
}

// Neumaier's compensated sum, one term at a time (srk_blur_weights_host's, as a value that can be read after every term).
namespace {
struct CompSum {
  double sum = 0.0, comp = 0.0;
  void add(double e) {
    const double t = sum + e;
    comp += fabs(sum) >= fabs(e) ? (sum - t) + e : (e - t) + sum;
    sum = t;
  }
  double value() const { return sum + comp; }
};
}  // namespace

extern "C" int srk_poisson_cdf_host(double peak, int KT, double* cdf) {
#pragma clang fp contract(off)
  SRK_REQUIRE(cdf, "poisson_cdf_host: null pointer");
  SRK_REQUIRE(KT >= 2, "poisson_cdf_host: KT must be at least 2 (got %d)", KT);
  SRK_REQUIRE(peak > 0.0 && peak <= 700.0, "poisson_cdf_host: peak must lie in (0, 700] (got %g)", peak);
  for (int L = 0; L < 256; ++L) {
    const double lambda = (double)L * peak / 255.0;
    double* row = cdf + (size_t)L * KT;
    double pmf = exp(-lambda), prev = 0.0;   // the running product pmf(k) = pmf(k - 1) * lambda / k
    CompSum s;
    for (int k = 0; k < KT; ++k) {
      if (k > 0) pmf = pmf * lambda / (double)k;
      s.add(pmf);
      double v = s.value();
      v = v > 1.0 ? 1.0 : v;
      v = v < prev ? prev : v;               // (a compensated sum of non-negative terms may still step back an ulp)
      row[k] = prev = v;
    }
    row[KT - 1] = 1.0;
  }
  return SRK_OK;
}

extern "C" int srk_blur_table_host(int kind, int K, double s1, double s2, double theta, double beta, double cutoff,
                                   double* w) {
#pragma clang fp contract(off)
  SRK_REQUIRE(w, "blur_table_host: null pointer");
  SRK_REQUIRE(kind >= SRK_BLUR_GAUSS && kind <= SRK_BLUR_SINC, "blur_table_host: unknown kind %d", kind);
  SRK_REQUIRE(K >= 7 && K <= kBlurMaxK && (K & 1), "blur_table_host: K must be odd and in [7, %d] (got %d)", kBlurMaxK, K);
  if (kind == SRK_BLUR_SINC) {
    SRK_REQUIRE(cutoff > 0.0, "blur_table_host: the sinc cutoff must be positive (got %g)", cutoff);
  } else {
    SRK_REQUIRE(s1 > 0.0 && s2 > 0.0, "blur_table_host: sigmas must be positive (got %g, %g)", s1, s2);
    SRK_REQUIRE(kind == SRK_BLUR_GAUSS || beta > 0.0, "blur_table_host: beta must be positive (got %g)", beta);
  }
  const int r = K / 2, n = K * K;
  const double c = cos(theta), s = sin(theta);
  for (int idx = 0; idx < n; ++idx) {
    const double xx = (double)(idx % K - r), yy = (double)(idx / K - r);
    if (kind == SRK_BLUR_SINC) {
      const double rr = sqrt(xx * xx + yy * yy);
      w[idx] = rr == 0.0 ? cutoff * cutoff / (4.0 * 3.141592653589793)
                         : cutoff * j1(cutoff * rr) / (2.0 * 3.141592653589793 * rr);
      continue;
    }
    const double u = c * xx + s * yy, v = -s * xx + c * yy;
    const double q = u * u / (s1 * s1) + v * v / (s2 * s2);
    w[idx] = kind == SRK_BLUR_GAUSS ? exp(-0.5 * q) : kind == SRK_BLUR_GGAUSS ? exp(-0.5 * pow(q, beta)) : 1.0 / (1.0 + pow(q, beta));
  }
  CompSum sum;
  for (int idx = 0; idx < n; ++idx) sum.add(w[idx]);
  const double total = sum.value();
  for (int idx = 0; idx < n; ++idx) w[idx] /= total;
  // `total` is itself rounded, so the divided table's sum can miss 1 by an ulp.  The centre tap (the largest of every
  // kind) takes up what is missing: (sum - 1) is exact so close to 1, the compensation carries the rest.
  CompSum again;
  for (int idx = 0; idx < n; ++idx) again.add(w[idx]);
  w[n / 2] -= (again.sum - 1.0) + again.comp;
  return SRK_OK;
}
