// A stand-alone run of srk_lpips_layer_host (csrc/lpips.hip, csrc/lpips_common.h) over the layer table of the tests, for
// the host sanitizers: it needs no device and no Python.  Build and run from the repo root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
//         pytorch_super_resolution_model_collection_amd/csrc/lpips.hip tools/lpips_host_check.cpp -o lpips_host_check && ./lpips_host_check
// Every buffer is allocated at its exact size, so a read or write past any of them is a report.  The program also checks
// the refusals (which must come before anything is read), that every result is finite with all-zero pixels planted in
// either map, the exact zeros of equal maps, and the planner's ranges; the numbers themselves are the CPU suite's
// business (tests/test_lpips_cpu.py).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../include/srk.h"

namespace srk {   // lpips.hip reports through the library's error slot (csrc/api.hip); this program keeps the last message
static char g_msg[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
}
}  // namespace srk

struct Case {
  int N, H, W, C;
};

static int run(const Case& c, bool backward, bool same) {
  std::mt19937 gen(4321u + (unsigned)c.N * 7 + (unsigned)c.C + (unsigned)c.H * 31);
  std::normal_distribution<float> nd(0.f, 1.f);
  const size_t pixels = (size_t)c.N * c.H * c.W, img = pixels * c.C;
  auto fill = [&](size_t n, bool relu) {
    std::vector<float> v(n);
    for (auto& e : v) {
      e = nd(gen);
      if (relu ? e < 0.f : false) e = 0.f;
      if (!relu) e = fabsf(e);
    }
    return v;
  };
  std::vector<float> f0 = fill(img, true), f1 = fill(img, true), w = fill(c.C, false);
  if (pixels >= 3) {   // all-zero pixels: in f0 only, in f1 only, in both
    for (int k = 0; k < c.C; ++k) f0[k] = 0.f, f1[(size_t)c.C + k] = 0.f, f0[(pixels - 1) * c.C + k] = f1[(pixels - 1) * c.C + k] = 0.f;
  }
  std::vector<double> g(backward ? c.N : 0), value(c.N), df0(backward ? img : 0);
  for (auto& e : g) e = nd(gen);
  const int rc = srk_lpips_layer_host(f0.data(), same ? f0.data() : f1.data(), w.data(), backward ? g.data() : nullptr, c.N,
                                      c.H, c.W, c.C, value.data(), backward ? df0.data() : nullptr);
  if (rc != SRK_OK) {
    printf("%d x %d x %d x %d: status %d (%s)\n", c.N, c.H, c.W, c.C, rc, srk::g_msg);
    return 1;
  }
  for (int n = 0; n < c.N; ++n)
    if (!isfinite(value[n]) || value[n] < 0.0 || (same && value[n] != 0.0)) {
      printf("%d x %d x %d x %d: value[%d] = %g\n", c.N, c.H, c.W, c.C, n, value[n]);
      return 1;
    }
  for (size_t i = 0; i < df0.size(); ++i)
    if (!isfinite(df0[i]) || (same && df0[i] != 0.0)) {
      printf("%d x %d x %d x %d: df0[%zu] = %g\n", c.N, c.H, c.W, c.C, i, df0[i]);
      return 1;
    }
  return 0;
}

int main() {
  const Case table[] = {{1, 1, 1, 1}, {2, 3, 5, 3}, {1, 4, 4, 64}, {2, 5, 7, 70}, {1, 2, 3, 128}, {3, 1, 9, 256}, {1, 3, 3, 512},
                        {1, 9, 8, 64}, {1, 2, 2, 2052}};
  int bad = 0;
  for (const Case& c : table)
    for (int backward = 0; backward < 2; ++backward)
      for (int same = 0; same < 2; ++same) bad += run(c, backward, same);
  // refusals come before any read: the pointers below are never dereferenced
  float one = 0.f;
  double out = 0.0;
  bad += srk_lpips_layer_host(nullptr, &one, &one, nullptr, 1, 1, 1, 4, &out, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_lpips_layer_host(&one, &one, &one, nullptr, 1, 1, 1, 4, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_lpips_layer_host(&one, &one, &one, nullptr, 0, 1, 1, 4, &out, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_lpips_layer_host(&one, &one, &one, nullptr, 1, 1, -1, 4, &out, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_lpips_layer_host(&one, &one, &one, nullptr, 1, 1, 1, 0, &out, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_lpips_layer_host(&one, &one, &one, &out, 1, 1, 1, 4, &out, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_lpips_layer_forward(&one, &one, &one, 1, 1, 1, 4, 5, 5, &out, &out, 1 << 20, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_lpips_layer_forward(&one, &one, &one, 1, 64, 64, 64, 0, 5, &out, &out, 8, nullptr) != SRK_ERR_WORKSPACE;
  bad += srk_lpips_layer_backward(&one, &one, &one, nullptr, 1, 1, 1, 4, &one, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_lpips_finish(nullptr, 5, 1, 1.0, &one, &one, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  // the planner: one block for a small map, several for a large one, capped, and the workspace covers both paths
  bad += srk_lpips_layer_blocks(1, 4, 4, 64, 1) != 1 || srk_lpips_layer_blocks(1, 128, 128, 64, 1) < 2;
  bad += srk_lpips_layer_blocks(1, 8000, 8000, 64, 1) != srk_lpips_layer_blocks(1, 4000, 4000, 64, 1);
  bad += srk_lpips_layer_blocks(1, 4, 4, 70, 1) != SRK_ERR_BAD_ARG;
  for (const Case& c : table) {
    int b = srk_lpips_layer_blocks(c.N, c.H, c.W, c.C, 0);
    if (c.C % 4 == 0 && srk_lpips_layer_blocks(c.N, c.H, c.W, c.C, 1) > b) b = srk_lpips_layer_blocks(c.N, c.H, c.W, c.C, 1);
    bad += b < 1 || srk_lpips_layer_workspace(c.N, c.H, c.W, c.C) < sizeof(double) * c.N * b;
  }
  printf(bad ? "lpips_host_check: %d FAILED\n" : "lpips_host_check: ok (%d failures)\n", bad);
  return bad != 0;
}
