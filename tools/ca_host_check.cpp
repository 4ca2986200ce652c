// A stand-alone run of srk_channel_attention_host (csrc/ca.hip, csrc/ca_common.h) over the case table of the tests, for
// the host sanitizers: it needs no device and no Python.  Build and run from the repo root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
//         pytorch_super_resolution_model_collection_amd/csrc/ca.hip tools/ca_host_check.cpp -o ca_host_check && ./ca_host_check
// Every buffer is allocated at its exact size, so a read or write past any of them is a report.  The program also checks
// the refusals (which must come before anything is read), that every result is finite, and the dead-hidden case's zeros;
// the numbers themselves are the CPU suite's business (tests/test_ca_cpu.py).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../include/srk.h"

namespace srk {   // ca.hip reports through the library's error slot (csrc/api.hip); this program keeps the last message
static char g_msg[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
}
}  // namespace srk

struct Case {
  const char* name;
  int N, C, Cr, H, W;
  int special;   // 1: b2 = +40 / -40, 2: b1 = -1e3
};

static int run(const Case& c, bool skip, bool backward) {
  std::mt19937 gen(1234u + (unsigned)c.N * 7 + (unsigned)c.C + (skip ? 100 : 0));
  std::normal_distribution<float> nd(0.f, 1.f);
  const size_t img = (size_t)c.N * c.H * c.W * c.C, nw = (size_t)c.C * c.Cr;
  auto fill = [&](size_t n, float std) {
    std::vector<float> v(n);
    for (auto& e : v) e = std * nd(gen);
    return v;
  };
  std::vector<float> t = fill(img, 1.f), x = fill(skip ? img : 0, 1.f), g = fill(img, 1.f);
  std::vector<float> w1 = fill(nw, .5f), b1 = fill(c.Cr, .5f), w2 = fill(nw, .5f), b2 = fill(c.C, .5f);
  if (c.special == 1)
    for (int i = 0; i < c.C; ++i) b2[i] = i < c.C / 2 ? 40.f : -40.f;
  if (c.special == 2)
    for (auto& e : b1) e = -1e3f;
  std::vector<double> y(img), dt(backward ? img : 0), dw1(backward ? nw : 0), db1(backward ? c.Cr : 0),
      dw2(backward ? nw : 0), db2(backward ? c.C : 0);
  const int rc = srk_channel_attention_host(t.data(), skip ? x.data() : nullptr, w1.data(), b1.data(), w2.data(), b2.data(),
                                            backward ? g.data() : nullptr, c.N, c.H, c.W, c.C, c.Cr, y.data(),
                                            backward ? dt.data() : nullptr, backward ? dw1.data() : nullptr,
                                            backward ? db1.data() : nullptr, backward ? dw2.data() : nullptr,
                                            backward ? db2.data() : nullptr);
  if (rc != SRK_OK) {
    printf("%s: status %d (%s)\n", c.name, rc, srk::g_msg);
    return 1;
  }
  for (size_t i = 0; i < img; ++i)
    if (!isfinite(y[i]) || (backward && !isfinite(dt[i]))) {
      printf("%s: element %zu is not finite\n", c.name, i);
      return 1;
    }
  if (c.special == 2 && backward)
    for (size_t i = 0; i < nw; ++i)
      if (dw1[i] != 0.0 || dw2[i] != 0.0) {
        printf("%s: a dead hidden layer left a weight gradient\n", c.name);
        return 1;
      }
  return 0;
}

int main() {
  const Case table[] = {{"hw1", 1, 4, 1, 1, 1, 0},       {"cr1", 2, 16, 1, 3, 5, 0},      {"scalar", 3, 6, 2, 7, 9, 0},
                        {"net_odd", 2, 64, 4, 17, 23, 0}, {"mid", 5, 32, 8, 8, 8, 0},      {"wide", 1, 64, 4, 96, 100, 0},
                        {"patch", 2, 64, 4, 40, 40, 0},   {"saturated", 2, 8, 2, 5, 6, 1}, {"dead_hidden", 2, 8, 2, 5, 6, 2},
                        {"limits", 1, 256, 64, 3, 3, 0}};
  int bad = 0;
  for (const Case& c : table)
    for (int skip = 0; skip < 2; ++skip)
      for (int backward = 0; backward < 2; ++backward) bad += run(c, skip, backward);
  // refusals come before any read: the pointers below are never dereferenced
  float one = 0.f;
  double out = 0.0;
  bad += srk_channel_attention_host(&one, nullptr, &one, &one, &one, &one, nullptr, 1, 1, 1, 257, 4, &out, nullptr, nullptr,
                                    nullptr, nullptr, nullptr) != SRK_ERR_UNSUPPORTED;
  bad += srk_channel_attention_host(&one, nullptr, &one, &one, &one, &one, nullptr, 1, 1, 1, 4, 5, &out, nullptr, nullptr,
                                    nullptr, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_channel_attention_host(nullptr, nullptr, &one, &one, &one, &one, nullptr, 1, 1, 1, 4, 2, &out, nullptr, nullptr,
                                    nullptr, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_channel_attention_splits(1, 96, 100, 64) < 2 || srk_channel_attention_splits(1, 1, 1, 4) != 1;
  printf(bad ? "ca_host_check: %d FAILED\n" : "ca_host_check: ok (%d failures)\n", bad);
  return bad != 0;
}
