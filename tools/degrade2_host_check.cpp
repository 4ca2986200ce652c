// A stand-alone run of the four host twins of the second-order degradation -- srk_blur_table_host, srk_poisson_cdf_host,
// srk_noise2_u8_host (csrc/degrade.hip, csrc/degrade_common.h) and srk_usm_u8_host with srk_usm_table_host (csrc/usm.hip,
// csrc/usm_common.h) -- for the host sanitizers: it needs no device and no Python.  Build and run from the repo root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
//         pytorch_super_resolution_model_collection_amd/csrc/degrade.hip pytorch_super_resolution_model_collection_amd/csrc/usm.hip
//         tools/degrade2_host_check.cpp -o degrade2_host_check && ./degrade2_host_check
// Every buffer is allocated at its exact size, so a read or write past any of them is a report.  The program also checks
// the refusals (which must come before anything is read), the tables' invariants and the identities; the bytes themselves
// are the CPU suite's business (tests/test_degrade2_cpu.py).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../include/srk.h"

namespace srk {   // the sources report through the library's error slot (csrc/api.hip); this program keeps the last message
static char g_msg[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
}
}  // namespace srk

static int g_fail = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++g_fail;                                                  \
    }                                                            \
  } while (0)

static std::vector<uint8_t> image(unsigned seed, size_t n) {
  std::mt19937 gen(seed);
  std::vector<uint8_t> v(n);
  for (auto& e : v) e = (uint8_t)(gen() & 255u);
  return v;
}

static void tables() {
  for (int kind = SRK_BLUR_GAUSS; kind <= SRK_BLUR_SINC; ++kind)
    for (int K = 7; K <= 21; K += 2) {
      std::vector<double> w((size_t)K * K);
      EXPECT(srk_blur_table_host(kind, K, 1.7, 0.6, 0.8, 1.5, 2.2, w.data()) == SRK_OK);
      double sum = 0.0, lo = 0.0;
      for (double e : w) sum += e, lo = e < lo ? e : lo;
      EXPECT(fabs(sum - 1.0) < 1e-13 && isfinite(sum));
      EXPECT((kind == SRK_BLUR_SINC) == (lo < 0.0));
    }
  std::vector<double> w(49);
  EXPECT(srk_blur_table_host(SRK_BLUR_GAUSS, 7, 1.0, 1.0, 0.0, 1.0, 1.0, nullptr) == SRK_ERR_INVALID);
  EXPECT(srk_blur_table_host(SRK_BLUR_GAUSS, 8, 1.0, 1.0, 0.0, 1.0, 1.0, w.data()) == SRK_ERR_INVALID);
  EXPECT(srk_blur_table_host(SRK_BLUR_GAUSS, 23, 1.0, 1.0, 0.0, 1.0, 1.0, w.data()) == SRK_ERR_INVALID);
  EXPECT(srk_blur_table_host(SRK_BLUR_SINC, 7, 1.0, 1.0, 0.0, 1.0, 0.0, w.data()) == SRK_ERR_INVALID);
  for (int K : {1, 5, 51}) {
    std::vector<double> g((size_t)K);
    EXPECT(srk_usm_table_host(K, 0.0, g.data()) == SRK_OK);
    double sum = 0.0;
    for (double e : g) sum += e;
    EXPECT(fabs(sum - 1.0) < 1e-14);
  }
  EXPECT(srk_usm_table_host(52, 0.0, w.data()) == SRK_ERR_INVALID && srk_usm_table_host(53, 0.0, w.data()) == SRK_ERR_INVALID);
}

static void noise(const std::vector<double>& cdf) {
  struct Shape { int B, C, H, W; };
  for (const Shape& s : {Shape{3, 3, 5, 7}, Shape{2, 1, 16, 16}, Shape{1, 3, 1, 1}}) {
    const size_t n = (size_t)s.B * s.C * s.H * s.W;
    const std::vector<uint8_t> x = image(7u + (unsigned)n, n);
    for (int mode = SRK_NOISE2_OFF; mode <= SRK_NOISE2_POISSON; ++mode)
      for (int gray = 0; gray < 2; ++gray)
        for (int color = 0; color < 2; ++color) {
          std::vector<double> m((size_t)s.B, (double)mode), g((size_t)s.B, (double)gray), a((size_t)s.B);
          for (int b = 0; b < s.B; ++b) a[b] = mode == SRK_NOISE2_GAUSS ? 30.0 * b : 3.0 - b;
          m[s.B - 1] = SRK_NOISE2_OFF;   // a patch that is left alone beside the others
          std::vector<uint8_t> y(n, 0), y2(n, 1);
          EXPECT(srk_noise2_u8_host(x.data(), y.data(), m.data(), g.data(), a.data(), cdf.data(), 0x9e3779b97f4a7c15ull, 1 + gray,
                                    s.B, s.C, s.H, s.W, color) == SRK_OK);
          EXPECT(srk_noise2_u8_host(x.data(), y2.data(), m.data(), g.data(), a.data(), cdf.data(), 0x9e3779b97f4a7c15ull, 1 + gray,
                                    s.B, s.C, s.H, s.W, color) == SRK_OK);
          EXPECT(y == y2);
          const size_t per = n / s.B;
          for (size_t e = n - per; e < n; ++e) EXPECT(y[e] == x[e]);
          if (mode == SRK_NOISE2_OFF) EXPECT(y == x);
        }
  }
  std::vector<uint8_t> x(48), y(48);
  std::vector<double> one(1, 1.0);
  EXPECT(srk_noise2_u8_host(nullptr, y.data(), one.data(), one.data(), one.data(), cdf.data(), 1, 1, 1, 3, 4, 4, 1) == SRK_ERR_INVALID);
  EXPECT(srk_noise2_u8_host(x.data(), y.data(), one.data(), one.data(), one.data(), nullptr, 1, 1, 1, 3, 4, 4, 1) == SRK_ERR_INVALID);
  EXPECT(srk_noise2_u8_host(x.data(), y.data(), one.data(), one.data(), one.data(), cdf.data(), 1, 1, 1, 2, 4, 4, 1) == SRK_ERR_INVALID);
  EXPECT(srk_noise2_u8_host(x.data(), y.data(), one.data(), one.data(), one.data(), cdf.data(), 1, 3, 1, 3, 4, 4, 1) == SRK_ERR_INVALID);
}

static void usm() {
  struct Shape { int B, C, H, W, K; };
  for (const Shape& s : {Shape{2, 3, 27, 40, 51}, Shape{1, 1, 64, 64, 51}, Shape{1, 3, 3, 3, 5}, Shape{1, 1, 1, 1, 1}}) {
    const size_t n = (size_t)s.B * s.C * s.H * s.W;
    const std::vector<uint8_t> x = image(11u + (unsigned)n, n);
    std::vector<double> g((size_t)s.K);
    EXPECT(srk_usm_table_host(s.K, 0.0, g.data()) == SRK_OK);
    std::vector<uint8_t> y(n, 0), same(n, 0);
    EXPECT(srk_usm_u8_host(x.data(), y.data(), g.data(), s.K, 0.5, 10.0, s.B, s.C, s.H, s.W) == SRK_OK);
    EXPECT(srk_usm_u8_host(x.data(), same.data(), g.data(), s.K, 0.5, 255.0, s.B, s.C, s.H, s.W) == SRK_OK);
    EXPECT(same == x);                       // nothing exceeds the threshold: the input
    const std::vector<uint8_t> flat(n, 137);
    EXPECT(srk_usm_u8_host(flat.data(), y.data(), g.data(), s.K, 0.5, 10.0, s.B, s.C, s.H, s.W) == SRK_OK);
    EXPECT(y == flat);                       // a constant plane returns itself
  }
  std::vector<uint8_t> x(3 * 26 * 26), y(3 * 26 * 26);
  std::vector<double> g(51);
  EXPECT(srk_usm_table_host(51, 0.0, g.data()) == SRK_OK);
  EXPECT(srk_usm_u8_host(x.data(), y.data(), g.data(), 51, 0.5, 10.0, 1, 3, 26, 26) == SRK_OK);
  EXPECT(srk_usm_u8_host(x.data(), y.data(), g.data(), 50, 0.5, 10.0, 1, 3, 26, 26) == SRK_ERR_INVALID);
  EXPECT(srk_usm_u8_host(x.data(), y.data(), g.data(), 53, 0.5, 10.0, 1, 3, 26, 26) == SRK_ERR_INVALID);
  EXPECT(srk_usm_u8_host(x.data(), y.data(), g.data(), 51, 0.5, 10.0, 1, 2, 26, 26) == SRK_ERR_INVALID);
  EXPECT(srk_usm_u8_host(x.data(), y.data(), g.data(), 51, 0.5, 10.0, 1, 3, 25, 26) == SRK_ERR_INVALID);
  EXPECT(srk_usm_u8_host(x.data(), nullptr, g.data(), 51, 0.5, 10.0, 1, 3, 26, 26) == SRK_ERR_INVALID);
}

int main() {
  tables();
  std::vector<double> cdf((size_t)256 * SRK_POISSON_KT);
  EXPECT(srk_poisson_cdf_host(256.0, SRK_POISSON_KT, cdf.data()) == SRK_OK);
  for (int L = 0; L < 256; ++L) {
    const double* row = cdf.data() + (size_t)L * SRK_POISSON_KT;
    for (int k = 1; k < SRK_POISSON_KT; ++k) EXPECT(row[k] >= row[k - 1]);
    EXPECT(row[SRK_POISSON_KT - 1] == 1.0 && row[SRK_POISSON_KT - 2] >= 1.0 - ldexp(1.0, -33));
  }
  EXPECT(srk_poisson_cdf_host(256.0, SRK_POISSON_KT, nullptr) == SRK_ERR_INVALID);
  EXPECT(srk_poisson_cdf_host(0.0, SRK_POISSON_KT, cdf.data()) == SRK_ERR_INVALID);
  noise(cdf);
  usm();
  printf(g_fail ? "degrade2_host_check: %d checks FAILED\n" : "degrade2_host_check: all checks passed\n", g_fail);
  return g_fail ? 1 : 0;
}
