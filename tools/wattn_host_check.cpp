// A stand-alone run of srk_window_attention_host (csrc/wattn.hip, csrc/wattn_common.h) over the case table of the tests,
// for the host sanitizers: it needs no device and no Python.  Build and run from the repo root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
//         pytorch_super_resolution_model_collection_amd/csrc/wattn.hip tools/wattn_host_check.cpp -o wattn_host_check
//   ./wattn_host_check
// Every buffer is allocated at its exact size, so a read or write past any of them is a report.  The program also checks
// the refusals (which must come before anything is read), that every result is finite, that every output element was
// written, that the rows of the softmax sum to one through a constant V, and the index functions' ranges; the numbers
// themselves are the CPU suite's business (tests/test_swinir_cpu.py).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../include/srk.h"

namespace srk {   // wattn.hip reports through the library's error slot (csrc/api.hip); this program keeps the last message
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
  int N, H, W, C, heads, window, shift;
};

static int run(const Case& c, bool backward) {
  std::mt19937 gen(99u + (unsigned)c.N * 7 + (unsigned)c.C);
  std::normal_distribution<float> nd(0.f, 1.f);
  const size_t pix = (size_t)c.N * c.H * c.W, bins = (size_t)(2 * c.window - 1) * (2 * c.window - 1);
  std::vector<float> qkv(pix * 3 * c.C), table(bins * c.heads), dout(pix * c.C);
  for (auto& e : qkv) e = nd(gen);
  for (auto& e : table) e = nd(gen);
  for (auto& e : dout) e = nd(gen);
  for (size_t p = 0; p < pix; ++p)   // V = 1 in the first channel of every head: that output channel is the row sum of P
    for (int h = 0; h < c.heads; ++h) qkv[p * 3 * c.C + 2 * c.C + h * (c.C / c.heads)] = 1.f;
  std::vector<double> out(pix * c.C, NAN), dqkv(backward ? pix * 3 * c.C : 0, NAN), dtable(backward ? bins * c.heads : 0, NAN);
  const int rc = srk_window_attention_host(qkv.data(), table.data(), backward ? dout.data() : nullptr, c.N, c.H, c.W, c.C,
                                           c.heads, c.window, c.shift, out.data(), backward ? dqkv.data() : nullptr,
                                           backward ? dtable.data() : nullptr);
  if (rc != SRK_OK) {
    printf("%s: status %d (%s)\n", c.name, rc, srk::g_msg);
    return 1;
  }
  int bad = 0;
  for (double v : out) bad += !isfinite(v);
  for (double v : dqkv) bad += !isfinite(v);
  for (double v : dtable) bad += !isfinite(v);
  for (size_t p = 0; p < pix; ++p)
    for (int h = 0; h < c.heads; ++h) bad += fabs(out[p * c.C + h * (c.C / c.heads)] - 1.0) > 1e-12;
  if (backward) {   // softmax rows sum to one: the gradient of the table sums to zero over each head
    for (int h = 0; h < c.heads; ++h) {
      double s = 0.0, a = 0.0;
      for (size_t b = 0; b < bins; ++b) s += dtable[b * c.heads + h], a += fabs(dtable[b * c.heads + h]);
      bad += fabs(s) > 1e-9 * (a + 1.0);
    }
  }
  printf("%-16s backward %d: %s\n", c.name, (int)backward, bad ? "BAD" : "ok");
  return bad != 0;
}

int main() {
  const Case cases[] = {{"one_window", 1, 4, 4, 4, 1, 4, 0},       {"2x3_windows", 2, 8, 12, 8, 2, 4, 2},
                        {"9_tokens", 1, 6, 9, 6, 2, 3, 1},         {"d30_classical", 2, 16, 16, 60, 2, 8, 4},
                        {"d10_lightweight", 1, 16, 24, 60, 6, 8, 4}, {"d32_shift3", 1, 16, 16, 64, 2, 8, 3},
                        {"4_tokens", 3, 8, 8, 16, 4, 2, 1}};
  int fails = 0;
  for (const Case& c : cases) fails += run(c, false) + run(c, true);
  // refusals come before any access: every pointer here is a one-float buffer
  float one = 0.f;
  double d1 = 0.0;
  const int bad_args[][7] = {{0, 4, 4, 4, 1, 4, 0},  {1, 9, 9, 4, 1, 9, 0}, {1, 4, 4, 4, 1, 1, 0}, {1, 4, 4, 4, 1, 4, 4},
                             {1, 4, 4, 4, 1, 4, -1}, {1, 6, 4, 4, 1, 4, 0}, {1, 4, 4, 6, 4, 4, 0}, {1, 4, 4, 33, 1, 4, 0}};
  for (const auto& a : bad_args) {
    const int rc = srk_window_attention_host(&one, &one, nullptr, a[0], a[1], a[2], a[3], a[4], a[5], a[6], &d1, nullptr,
                                             nullptr);
    if (rc != SRK_ERR_BAD_ARG) printf("refusal missed: %d %d %d %d %d %d %d -> %d\n", a[0], a[1], a[2], a[3], a[4], a[5], a[6], rc), ++fails;
  }
  if (srk_window_attention_host(&one, &one, &one, 1, 4, 4, 4, 1, 4, 0, &d1, nullptr, nullptr) != SRK_ERR_BAD_ARG) ++fails;
  // the index functions stay in range over every window size and shift
  for (int w = 2; w <= 8; ++w)
    for (int s = 0; s < w; ++s) {
      const int H = 2 * w, W = 3 * w;
      for (int i = 0; i < w * w; ++i)
        for (int j = 0; j < w * w; ++j) {
          const int r = srk_window_attention_rel_index(w, i, j);
          fails += r < 0 || r >= (2 * w - 1) * (2 * w - 1);
        }
      std::vector<int> seen((size_t)H * W, 0);
      for (int wy = 0; wy < 2; ++wy)
        for (int wx = 0; wx < 3; ++wx)
          for (int t = 0; t < w * w; ++t) {
            const int64_t p = srk_window_attention_token_pixel(H, W, w, s, wy, wx, t);
            if (p < 0 || p >= (int64_t)H * W) ++fails;
            else ++seen[(size_t)p];
          }
      for (int v : seen) fails += v != 1;   // the windows tile the picture: every pixel exactly once
      for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
          const int id = srk_window_attention_region(H, W, w, s, r, c);
          fails += id < 0 || id > 8 || (s == 0 && id != 0);
        }
    }
  fails += srk_window_attention_rel_index(9, 0, 0) != -1 || srk_window_attention_region(8, 8, 4, 2, 8, 0) != -1 ||
           srk_window_attention_token_pixel(8, 8, 4, 2, 2, 0, 0) != -1;
  printf(fails ? "FAILED (%d)\n" : "all clean\n", fails);
  return fails != 0;
}
