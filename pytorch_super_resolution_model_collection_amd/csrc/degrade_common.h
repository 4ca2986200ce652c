// What the noise kernel (degrade.hip: k_noise_u8) and its host twin (srk_noise_normals_host) share: Philox4x32-10 and the
// Box-Muller step that makes four normals of its four words.  One body, compiled for both sides.  DESIGN.md 23.
#ifndef SRK_DEGRADE_COMMON_H_
#define SRK_DEGRADE_COMMON_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace srk {

constexpr int kBlurMaxK = 21;   // widest blur table: 2 * ceil(3 * sigma) + 1 capped here (sigma 4 -> 25 -> 21)

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): ten rounds on the counter c[0..3] under the key (k0, k1), the key
// bumped by the Weyl constants between rounds.
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// The four words of group q under `seed`: key (seed & 0xffffffff, seed >> 32), counter (q & 0xffffffff, q >> 32, 0, 0).
__host__ __device__ __forceinline__ void noise_words(uint64_t seed, uint64_t q, uint32_t x[4]) {
  x[0] = (uint32_t)q;
  x[1] = (uint32_t)(q >> 32);
  x[2] = 0u;
  x[3] = 0u;
  philox4x32_10(x, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// u(x) = (x + 0.5) * 2^-32, in (0, 1): the logarithm below is finite for every word.
__host__ __device__ __forceinline__ double noise_unit(uint32_t x) { return ((double)x + 0.5) * (1.0 / 4294967296.0); }

// Box-Muller in fp64: words (x0, x1) -> n[0], n[1], words (x2, x3) -> n[2], n[3].  Element e of a tensor takes lane e & 3
// of group e >> 2.
__host__ __device__ __forceinline__ void noise_normals4(uint64_t seed, uint64_t q, double n[4]) {
  uint32_t x[4];
  noise_words(seed, q, x);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const double rad = sqrt(-2.0 * log(noise_unit(x[2 * h])));
    const double ang = 6.283185307179586 * noise_unit(x[2 * h + 1]);
    n[2 * h] = rad * cos(ang);
    n[2 * h + 1] = rad * sin(ang);
  }
}

// ---- the second-order chain's noise (srk_noise2_u8) ----------------------------------------------------
constexpr int kNoise2Off = 0, kNoise2Gauss = 1, kNoise2Poisson = 2;
constexpr int kPoissonKT = 448;   // columns of the Poisson table cdf[256][KT]: the mass beyond is below 2^-32

// noise_words with the stage number (0: srk_noise_u8's own stream, 1 / 2: the chain's stages) in counter word 2.
__host__ __device__ __forceinline__ void noise2_words(uint64_t seed, uint64_t q, uint32_t stage, uint32_t x[4]) {
  x[0] = (uint32_t)q;
  x[1] = (uint32_t)(q >> 32);
  x[2] = stage;
  x[3] = 0u;
  philox4x32_10(x, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Lane `lane` of the four Box-Muller normals of the words x (noise_normals4's arithmetic, one lane of it).
__host__ __device__ __forceinline__ double noise2_normal(const uint32_t x[4], int lane) {
  const int h = lane >> 1;
  const double rad = sqrt(-2.0 * log(noise_unit(x[2 * h])));
  const double ang = 6.283185307179586 * noise_unit(x[2 * h + 1]);
  return (lane & 1) ? rad * sin(ang) : rad * cos(ang);
}

// The Poisson count of level L under the word: the smallest k with u(word) <= cdf[L][k].  The last column is 1.0 and
// u < 1, so the search ends inside the row.
__host__ __device__ __forceinline__ int noise2_poisson_k(const double* __restrict__ cdf, int L, uint32_t word) {
  const double u = noise_unit(word);
  const double* row = cdf + (size_t)L * kPoissonKT;
  int lo = 0, hi = kPoissonKT - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (u <= row[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__host__ __device__ __forceinline__ uint8_t noise2_round(double v) {
  const double r = floor(v + 0.5);
  return (uint8_t)(int)fmin(fmax(r, 0.0), 255.0);
}

// Elements e0 .. e0 + n - 1 (n <= 4, one Philox group of the colour stream) of dense 8-bit x [B][C][HW] -> y.  Colour
// noise indexes the generator by the element, gray noise by the pixel b * HW + p: lane (index & 3) of group (index >> 2).
// The group's words are kept while consecutive elements stay inside it.  Products and sums are not contracted, so
// the host and the device make the same roundings.
__host__ __device__ __forceinline__ void noise2_group(const uint8_t* __restrict__ x, uint8_t* __restrict__ y,
                                                      const double* __restrict__ mode, const double* __restrict__ gray,
                                                      const double* __restrict__ amount, const double* __restrict__ cdf,
                                                      uint64_t seed, uint32_t stage, int C, int64_t HW, int color, int64_t e0,
                                                      int n) {
#pragma clang fp contract(off)
  uint32_t words[4] = {0u, 0u, 0u, 0u};
  int64_t have = -1;
  for (int k = 0; k < n; ++k) {
    const int64_t e = e0 + k;
    const int64_t plane = e / HW, p = e - plane * HW;
    const int64_t b = plane / C;
    const int m = (int)mode[b];
    const double L = (double)x[e];
    if (m != kNoise2Gauss && m != kNoise2Poisson) {
      y[e] = x[e];
      continue;
    }
    const bool g = gray[b] != 0.0;
    const int64_t idx = g ? b * HW + p : e;
    if ((idx >> 2) != have) {   // (the words depend on the group's number alone, whichever rule numbered it)
      have = idx >> 2;
      noise2_words(seed, (uint64_t)have, stage, words);
    }
    const int lane = (int)(idx & 3);
    const double a = amount[b];
    if (m == kNoise2Gauss) {
      y[e] = noise2_round(L + a * noise2_normal(words, lane));
      continue;
    }
    double Lg = L;
    if (g && C == 3) {   // the pixel's gray level: the mean of R, G, B, or of Y, Cb, Cr planes the Y plane
      const uint8_t* px = x + b * 3 * HW + p;
      Lg = color ? floor((double)((int)px[0] + (int)px[HW] + (int)px[2 * HW]) / 3.0 + 0.5) : (double)px[0];
    }
    const int kk = noise2_poisson_k(cdf, (int)Lg, words[lane]);
    const double d = (double)kk * 255.0 / 256.0 - Lg;
    y[e] = noise2_round(L + a * d);
  }
}

}  // namespace srk
#endif  // SRK_DEGRADE_COMMON_H_
