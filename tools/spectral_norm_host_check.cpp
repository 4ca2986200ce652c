// A stand-alone run of the host twins of Real-ESRGAN's discriminator operators -- srk_spectral_norm_host
// (csrc/spectral_norm.hip), srk_upsample_bilinear2x_host (csrc/bilinear.hip), srk_gan_logit_loss_host (csrc/gan_logit.hip)
// -- over the case tables of the tests, for the host sanitizers: it needs no device and no Python.  Build and run from the
// repo root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
//         pytorch_super_resolution_model_collection_amd/csrc/spectral_norm.hip
//         pytorch_super_resolution_model_collection_amd/csrc/bilinear.hip
//         pytorch_super_resolution_model_collection_amd/csrc/gan_logit.hip tools/spectral_norm_host_check.cpp
//         -o spectral_norm_host_check
//   ./spectral_norm_host_check
// Every buffer is allocated at its exact size, so a read or write past any of them is a report.  The program also checks
// the refusals (which must come before anything is read), that every result is finite, that every output element was
// written, that u and v leave a training-mode call as unit vectors and an eval-mode call untouched, that sigma times w_sn
// gives W back, and the adjoint identity of the upsampling; the numbers themselves are the CPU suite's business
// (tests/test_realesrgan_cpu.py).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../include/srk.h"

namespace srk {   // the .hip files report through the library's error slot (csrc/api.hip); this program keeps the last message
static char g_msg[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
}
}  // namespace srk

static std::mt19937 gen(2021u);
static std::normal_distribution<float> nd(0.f, 1.f);

static int count_bad(const std::vector<double>& v) {
  int bad = 0;
  for (double e : v) bad += !isfinite(e);
  return bad;
}

static int run_sn(int R, int K, int training) {
  std::vector<float> W((size_t)R * K);
  for (auto& e : W) e = nd(gen) * sqrtf(2.f / K);
  std::vector<double> u(R), v(K), G((size_t)R * K);
  double nu = 0, nv = 0;
  for (auto& e : u) e = nd(gen), nu += e * e;
  for (auto& e : v) e = nd(gen), nv += e * e;
  for (auto& e : u) e /= sqrt(nu);
  for (auto& e : v) e /= sqrt(nv);
  for (auto& e : G) e = nd(gen);
  const std::vector<double> u0 = u, v0 = v;
  std::vector<double> w_sn((size_t)R * K, NAN), dW((size_t)R * K, NAN);
  double sigma = NAN;
  int rc = srk_spectral_norm_host(W.data(), R, K, training, 1e-12, u.data(), v.data(), w_sn.data(), &sigma, G.data(), dW.data());
  if (rc != SRK_OK) {
    printf("spectral_norm %dx%d: status %d (%s)\n", R, K, rc, srk::g_msg);
    return 1;
  }
  int bad = count_bad(w_sn) + count_bad(dW) + count_bad(u) + count_bad(v) + !isfinite(sigma);
  if (training) {
    nu = nv = 0;
    for (double e : u) nu += e * e;
    for (double e : v) nv += e * e;
    bad += fabs(nu - 1.0) > 1e-12 || fabs(nv - 1.0) > 1e-12;
  } else {
    bad += u != u0 || v != v0;
  }
  for (size_t i = 0; i < W.size(); ++i) bad += fabs(w_sn[i] * sigma - (double)W[i]) > 1e-12 * (fabs((double)W[i]) + 1e-30);
  // forward only: G and dW both NULL
  std::vector<double> w2((size_t)R * K, NAN);
  std::vector<double> u2 = u0, v2 = v0;
  rc = srk_spectral_norm_host(W.data(), R, K, training, 1e-12, u2.data(), v2.data(), w2.data(), &sigma, nullptr, nullptr);
  bad += rc != SRK_OK || w2 != w_sn;
  printf("spectral_norm %4d x %-5d %s: %s\n", R, K, training ? "train" : "eval ", bad ? "BAD" : "ok");
  return bad != 0;
}

static int run_bilinear(int N, int H, int W, int C, bool with_add) {
  const size_t in = (size_t)N * H * W * C, out = in * 4;
  std::vector<float> x(in), add(with_add ? in : 0), dy(out);
  for (auto& e : x) e = nd(gen);
  for (auto& e : add) e = nd(gen);
  for (auto& e : dy) e = nd(gen);
  std::vector<double> y(out, NAN), dx(in, NAN);
  const int rc = srk_upsample_bilinear2x_host(x.data(), with_add ? add.data() : nullptr, dy.data(), N, H, W, C, y.data(), dx.data());
  if (rc != SRK_OK) {
    printf("bilinear %d %d %d %d: status %d (%s)\n", N, H, W, C, rc, srk::g_msg);
    return 1;
  }
  int bad = count_bad(y) + count_bad(dx);
  double lhs = 0, rhs = 0, mag = 0;
  for (size_t i = 0; i < out; ++i) lhs += y[i] * dy[i], mag += fabs(y[i] * dy[i]);
  for (size_t i = 0; i < in; ++i) rhs += ((double)x[i] + (with_add ? (double)add[i] : 0.0)) * dx[i];
  bad += fabs(lhs - rhs) > 1e-12 * (mag + 1.0);
  // each half alone
  std::vector<double> y2(out, NAN), dx2(in, NAN);
  bad += srk_upsample_bilinear2x_host(x.data(), with_add ? add.data() : nullptr, nullptr, N, H, W, C, y2.data(), nullptr) != SRK_OK;
  bad += srk_upsample_bilinear2x_host(nullptr, nullptr, dy.data(), N, H, W, C, nullptr, dx2.data()) != SRK_OK;
  bad += y2 != y || dx2 != dx;
  printf("bilinear2x %d x %d x %d x %-3d %s: %s\n", N, H, W, C, with_add ? "add  " : "plain", bad ? "BAD" : "ok");
  return bad != 0;
}

static int run_gan(size_t n, int real) {
  std::vector<float> x(n);
  for (auto& e : x) e = 2.f * nd(gen);
  x[0] = 60.f;
  x[n - 1] = -60.f;
  std::vector<double> dx(n, NAN);
  double loss = NAN, loss2 = NAN;
  int rc = srk_gan_logit_loss_host(x.data(), n, real, 0.25, &loss, dx.data());
  int bad = rc != SRK_OK || !isfinite(loss) || loss < 0.0 || count_bad(dx);
  rc = srk_gan_logit_loss_host(x.data(), n, real, 0.25, &loss2, nullptr);
  bad += rc != SRK_OK || loss2 != loss;
  printf("gan_logit_loss n = %-6zu %s: %s\n", n, real ? "real" : "fake", bad ? "BAD" : "ok");
  return bad != 0;
}

int main() {
  int fails = 0;
  const int sn[][2] = {{1, 1}, {1, 7}, {5, 1}, {3, 27}, {16, 48}, {64, 576}, {130, 117}, {128, 1024}, {512, 4096}};
  for (const auto& s : sn) fails += run_sn(s[0], s[1], 1) + run_sn(s[0], s[1], 0);
  const int bl[][4] = {{1, 1, 1, 1}, {1, 1, 5, 3}, {1, 4, 1, 2}, {2, 2, 2, 1}, {2, 3, 5, 7}, {1, 8, 8, 64}, {2, 5, 9, 130}};
  for (const auto& b : bl) fails += run_bilinear(b[0], b[1], b[2], b[3], false) + run_bilinear(b[0], b[1], b[2], b[3], true);
  const size_t gn[] = {1, 3, 255, 256, 257, 4097, 65536};
  for (size_t n : gn) fails += run_gan(n, 1) + run_gan(n, 0);
  // refusals come before any access: every pointer here is a one-element buffer
  float one = 0.f;
  double d1 = 0.0;
  const int bad_sn[][2] = {{0, 4}, {4, 0}, {-1, 4}, {4, -3}};
  for (const auto& a : bad_sn)
    fails += srk_spectral_norm_host(&one, a[0], a[1], 1, 1e-12, &d1, &d1, &d1, &d1, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  fails += srk_spectral_norm_host(&one, 4, 4, 1, -1.0, &d1, &d1, &d1, &d1, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  fails += srk_spectral_norm_host(&one, 4, 4, 1, 1e-12, &d1, &d1, &d1, &d1, &d1, nullptr) != SRK_ERR_BAD_ARG;
  fails += srk_spectral_norm_host(&one, 4, 4, 1, 1e-12, &d1, &d1, &d1, &d1, nullptr, &d1) != SRK_ERR_BAD_ARG;
  fails += srk_spectral_norm_host(nullptr, 4, 4, 1, 1e-12, &d1, &d1, &d1, &d1, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  fails += srk_spectral_norm_host(&one, 4, 4, 1, 1e-12, &d1, &d1, &d1, nullptr, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  const int bad_bl[][4] = {{0, 2, 2, 1}, {1, 0, 2, 1}, {1, 2, -1, 1}, {1, 2, 2, 0}};
  for (const auto& a : bad_bl)
    fails += srk_upsample_bilinear2x_host(&one, nullptr, &one, a[0], a[1], a[2], a[3], &d1, &d1) != SRK_ERR_BAD_ARG;
  fails += srk_upsample_bilinear2x_host(&one, nullptr, nullptr, 1, 2, 2, 1, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  fails += srk_upsample_bilinear2x_host(nullptr, nullptr, nullptr, 1, 2, 2, 1, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  fails += srk_upsample_bilinear2x_host(nullptr, &one, &one, 1, 2, 2, 1, nullptr, &d1) != SRK_ERR_BAD_ARG;
  fails += srk_upsample_bilinear2x_host(&one, nullptr, &one, 1, 2, 2, 1, &d1, nullptr) != SRK_ERR_BAD_ARG;
  fails += srk_gan_logit_loss_host(&one, 0, 1, 1.0, &d1, nullptr) != SRK_ERR_BAD_ARG;
  fails += srk_gan_logit_loss_host(nullptr, 4, 1, 1.0, &d1, nullptr) != SRK_ERR_BAD_ARG;
  fails += srk_gan_logit_loss_host(&one, 4, 0, 1.0, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  printf(fails ? "FAILED (%d)\n" : "all clean\n", fails);
  return fails != 0;
}
