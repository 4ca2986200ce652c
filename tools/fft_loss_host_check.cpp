// A stand-alone run of srk_fft_loss_host and srk_dft_table_host (csrc/fft_loss.hip, csrc/fft_loss_common.h) over the
// shapes of the tests' case table, for the host sanitizers: it needs no device and no Python.  Build and run from the
// repo root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
//         pytorch_super_resolution_model_collection_amd/csrc/fft_loss.hip tools/fft_loss_host_check.cpp
//         -o fft_loss_host_check && ./fft_loss_host_check
// Every buffer is allocated at its exact size, so a read or write past any of them is a report.  The program also checks
// the refusals (which must come before anything is read), the exact table entries, that every result is finite, the
// identical pair's exact zeros and that a strided target gives the bits of a dense one; the numbers themselves are the
// CPU suite's business (tests/test_fft_loss_cpu.py).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../include/srk.h"

namespace srk {   // fft_loss.hip reports through the library's error slot (csrc/api.hip); this program keeps the last message
static char g_msg[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
}
}  // namespace srk

struct Case {
  int N, C, H, W;
};

static int run(const Case& c, bool ortho, bool backward, bool identical) {
  std::mt19937 gen(1234u + (unsigned)c.N * 7 + (unsigned)c.C + (unsigned)c.H * 31 + (unsigned)c.W);
  std::uniform_real_distribution<float> ud(0.f, 1.f);
  std::normal_distribution<float> nd(0.f, 1.f);
  const size_t m = (size_t)c.N * c.C * c.H * c.W;
  std::vector<float> t(m), p(m);                         // both NHWC-dense
  for (size_t i = 0; i < m; ++i) t[i] = ud(gen), p[i] = identical ? t[i] : t[i] + 0.1f * nd(gen);
  // the same target as NCHW, addressed through strides
  std::vector<float> tn(m);
  for (int n = 0; n < c.N; ++n)
    for (int y = 0; y < c.H; ++y)
      for (int x = 0; x < c.W; ++x)
        for (int ch = 0; ch < c.C; ++ch)
          tn[(((size_t)n * c.C + ch) * c.H + y) * c.W + x] = t[(((size_t)n * c.H + y) * c.W + x) * c.C + ch];
  const int64_t nchw[4] = {(int64_t)c.C * c.H * c.W, (int64_t)c.H * c.W, c.W, 1};
  const double scale = ortho ? 1.0 / sqrt((double)c.H * c.W) : 1.0;
  std::vector<double> g(backward ? m : 0), g2(backward ? m : 0);
  double loss = -1.0, loss2 = -2.0;
  int rc = srk_fft_loss_host(p.data(), t.data(), nullptr, c.N, c.C, c.H, c.W, scale, 1.0, &loss, backward ? g.data() : nullptr);
  if (rc == SRK_OK)
    rc = srk_fft_loss_host(p.data(), tn.data(), nchw, c.N, c.C, c.H, c.W, scale, 1.0, &loss2, backward ? g2.data() : nullptr);
  if (rc != SRK_OK) {
    printf("%d x %d x %d x %d: status %d (%s)\n", c.N, c.C, c.H, c.W, rc, srk::g_msg);
    return 1;
  }
  int bad = !isfinite(loss) || loss != loss2 || (identical ? loss != 0.0 : !(loss > 0.0));
  for (size_t i = 0; i < g.size(); ++i) bad += !isfinite(g[i]) || g[i] != g2[i] || (identical && g[i] != 0.0);
  if (bad) printf("%d x %d x %d x %d: %d wrong values (loss %g, %g)\n", c.N, c.C, c.H, c.W, bad, loss, loss2);
  return bad != 0;
}

static int tables() {
  int bad = 0;
  for (int n : {1, 2, 4, 7, 8, 12, 41, 256}) {
    std::vector<double> t((size_t)2 * n);
    bad += srk_dft_table_host(n, t.data()) != SRK_OK;
    for (int k = 0; k < n; ++k) {
      const double c = t[2 * k], s = t[2 * k + 1];
      const bool exact = (c == 0.0 || c == 1.0 || c == -1.0) && (s == 0.0 || s == 1.0 || s == -1.0);
      bad += exact != ((4 * k) % n == 0);
      bad += fabs(c * c + s * s - 1.0) > 4e-16;
      if (k) bad += t[2 * (n - k)] != c || t[2 * (n - k) + 1] != -s;
    }
  }
  double one = 0.0;
  bad += srk_dft_table_host(0, &one) != SRK_ERR_BAD_ARG;
  bad += srk_dft_table_host(4, nullptr) != SRK_ERR_BAD_ARG;
  if (bad) printf("tables: %d wrong entries\n", bad);
  return bad;
}

int main() {
  const Case table[] = {{1, 1, 1, 1},   {1, 1, 1, 7},   {2, 1, 2, 2},     {1, 3, 8, 8},    {2, 3, 7, 5},
                        {1, 1, 6, 10},  {2, 5, 16, 16}, {1, 3, 17, 33},   {2, 1, 41, 41},  {1, 3, 48, 64},
                        {1, 1, 128, 128}, {1, 2, 130, 66}, {1, 1, 256, 256}, {1, 1, 256, 3}};
  int bad = tables();
  for (const Case& c : table)
    for (int backward = 0; backward < 2; ++backward) bad += run(c, false, backward, false);
  bad += run({2, 3, 16, 24}, true, true, false);
  bad += run({2, 3, 16, 12}, false, true, true);
  // refusals come before any read: the pointers below are never dereferenced
  float one = 0.f;
  double out = 0.0;
  bad += srk_fft_loss_host(&one, &one, nullptr, 1, 1, 257, 4, 1.0, 1.0, &out, nullptr) != SRK_ERR_UNSUPPORTED;
  bad += srk_fft_loss_host(&one, &one, nullptr, 1, 1, 4, 257, 1.0, 1.0, &out, nullptr) != SRK_ERR_UNSUPPORTED;
  bad += srk_fft_loss_host(&one, &one, nullptr, 1, 0, 4, 4, 1.0, 1.0, &out, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_fft_loss_host(nullptr, &one, nullptr, 1, 1, 4, 4, 1.0, 1.0, &out, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_fft_loss_host(&one, &one, nullptr, 1, 1, 4, 4, 0.0, 1.0, &out, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_fft_loss_host(&one, &one, nullptr, 1, 1, 4, 4, 1.0, 1.0, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_fft_loss_forward_backward(&one, &one, nullptr, 1, 1, 257, 4, &out, 1.0, 1.f, &one, nullptr, &one, nullptr) !=
         SRK_ERR_UNSUPPORTED;
  bad += srk_fft_loss_workspace_bytes(1, 1, 257, 4) != 0 || srk_fft_loss_workspace_bytes(1, 3, 32, 32) < 2 * 3 * 32 * 17 * 16;
  printf(bad ? "fft_loss_host_check: %d FAILED\n" : "fft_loss_host_check: ok (%d failures)\n", bad);
  return bad != 0;
}
