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

}  // namespace srk
#endif  // SRK_DEGRADE_COMMON_H_
