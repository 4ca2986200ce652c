// A stand-alone run of srk_vgg_tap_forward_host / srk_vgg_tap_backward_host (csrc/vgg_tap.hip, csrc/vgg_tap_common.h) over
// the operator table of the tests, for the host sanitizers: it needs no device and no Python.  Build and run from the repo
// root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
//         pytorch_super_resolution_model_collection_amd/csrc/vgg_tap.hip tools/vgg_tap_host_check.cpp -o vgg_tap_host_check
//         && ./vgg_tap_host_check
// Every buffer is allocated at its exact size, so a read or write past any of them is a report.  The program also checks
// that every output element is written (NaN pre-fill), the exact zeros of equal maps, that a window without a positive
// value routes nothing, the refusals (which must come before anything is read) and the planner's ranges; the numbers
// themselves are the CPU suite's business (tests/test_vgg_taps_cpu.py).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../include/srk.h"

namespace srk {   // vgg_tap.hip reports through the library's error slot (csrc/api.hip); this program keeps the last message
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

static int fail(const Case& c, int mode, const char* what, size_t i, double v) {
  printf("%d x %d x %d x %d mode %d: %s[%zu] = %g\n", c.N, c.C, c.H, c.W, mode, what, i, v);
  return 1;
}

static int run(const Case& c, int mode, bool same, bool dead) {
  std::mt19937 gen(977u + (unsigned)c.N * 7 + (unsigned)c.C + (unsigned)c.H * 31 + (unsigned)mode);
  std::normal_distribution<float> nd(0.f, 1.f);
  const size_t total = (size_t)c.N * c.H * c.W * c.C;
  const bool pool = mode == SRK_VGG_TAP_POOL, last = mode == SRK_VGG_TAP_LAST;
  const size_t outs = last ? 0 : (pool ? (size_t)c.N * (c.H / 2) * (c.W / 2) * c.C : total);
  std::vector<float> a(total), b(total), g(outs), ya(outs, NAN), yb(outs, NAN), da(total, NAN);
  for (auto& e : a) e = dead ? -fabsf(nd(gen)) : nd(gen);
  for (auto& e : b) e = nd(gen);
  for (auto& e : g) e = nd(gen);
  const float* bp = same ? a.data() : b.data();
  double loss = NAN;
  int rc = srk_vgg_tap_forward_host(a.data(), bp, c.N, c.H, c.W, c.C, mode, 0.7, &loss, last ? nullptr : ya.data(),
                                    last ? nullptr : yb.data());
  if (rc == SRK_OK)
    rc = srk_vgg_tap_backward_host(a.data(), bp, last ? nullptr : g.data(), c.N, c.H, c.W, c.C, mode, 0.7 / (double)total,
                                   da.data());
  if (rc != SRK_OK) {
    printf("%d x %d x %d x %d mode %d: status %d (%s)\n", c.N, c.C, c.H, c.W, mode, rc, srk::g_msg);
    return 1;
  }
  if (!isfinite(loss) || loss < 0.0 || (same && loss != 0.0)) return fail(c, mode, "loss", 0, loss);
  for (size_t i = 0; i < outs; ++i) {
    if (!isfinite(ya[i]) || ya[i] < 0.f || (dead && ya[i] != 0.f)) return fail(c, mode, "ya", i, ya[i]);
    if (!isfinite(yb[i]) || yb[i] < 0.f || (same && yb[i] != ya[i])) return fail(c, mode, "yb", i, yb[i]);
  }
  for (size_t i = 0; i < total; ++i) {
    if (!isfinite(da[i])) return fail(c, mode, "da", i, da[i]);
    // nothing positive anywhere: the map behind the tap routes nothing, what is left is c * sign(a - b)
    const double want = same ? 0.0 : 0.7 / (double)total;   // (stored as fp32)
    if (dead && fabs(fabs((double)da[i]) - want) > 1e-6 * want) return fail(c, mode, "da (dead)", i, da[i]);
  }
  return 0;
}

int main() {
  const Case table[] = {{1, 1, 2, 2}, {1, 3, 2, 3}, {1, 4, 3, 2}, {1, 5, 7, 9}, {2, 8, 6, 10}, {1, 64, 2, 2}, {2, 64, 34, 38}};
  const Case one = {1, 512, 1, 1};
  int bad = 0;
  for (const Case& c : table)
    for (int mode = 0; mode < 3; ++mode)
      for (int same = 0; same < 2; ++same)
        for (int dead = 0; dead < 2; ++dead) bad += run(c, mode, same, dead);
  bad += run(one, SRK_VGG_TAP_LAST, false, false) + run(one, SRK_VGG_TAP_LAST, true, true);
  // refusals come before any read: the pointers below are never dereferenced
  float f = 0.f;
  double out = 0.0;
  bad += srk_vgg_tap_forward_host(nullptr, &f, 1, 2, 2, 4, SRK_VGG_TAP_POOL, 1.0, &out, &f, &f) != SRK_ERR_BAD_ARG;
  bad += srk_vgg_tap_forward_host(&f, &f, 1, 2, 2, 4, SRK_VGG_TAP_POOL, 1.0, nullptr, &f, &f) != SRK_ERR_BAD_ARG;
  bad += srk_vgg_tap_forward_host(&f, &f, 1, 2, 2, 4, SRK_VGG_TAP_POOL, 1.0, &out, nullptr, &f) != SRK_ERR_BAD_ARG;
  bad += srk_vgg_tap_forward_host(&f, &f, 0, 2, 2, 4, SRK_VGG_TAP_POOL, 1.0, &out, &f, &f) != SRK_ERR_BAD_ARG;
  bad += srk_vgg_tap_forward_host(&f, &f, 1, 1, 2, 4, SRK_VGG_TAP_POOL, 1.0, &out, &f, &f) != SRK_ERR_BAD_ARG;
  bad += srk_vgg_tap_forward_host(&f, &f, 1, 2, 2, 4, 7, 1.0, &out, &f, &f) != SRK_ERR_BAD_ARG;
  bad += srk_vgg_tap_forward_host(&f, &f, 1, 2, 2, 4, SRK_VGG_TAP_POOL, -1.0, &out, &f, &f) != SRK_ERR_BAD_ARG;
  bad += srk_vgg_tap_backward_host(&f, &f, nullptr, 1, 2, 2, 4, SRK_VGG_TAP_RELU, 1.0, &f) != SRK_ERR_BAD_ARG;
  bad += srk_vgg_tap_backward_host(&f, &f, &f, 1, 2, 2, 4, SRK_VGG_TAP_RELU, 1.0, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_vgg_tap_forward(&f, &f, 1, 2, 2, 4, SRK_VGG_TAP_POOL, 1.0, 1, 1, &out, &f, &f, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_vgg_tap_backward(&f, &f, nullptr, 1, 2, 2, 4, SRK_VGG_TAP_POOL, 1.0, nullptr, &f, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_vgg_tap_finish(nullptr, 1, &f, nullptr) != SRK_ERR_BAD_ARG;
  // the planner: one block for a small map, several for a large one, capped by the slots of a workspace row
  long long items = 0;
  const int slots = (int)(srk_vgg_tap_workspace_bytes(1) / sizeof(double));
  bad += srk_vgg_tap_workspace_bytes(0) != 0 || slots < 1 || srk_vgg_tap_workspace_bytes(5) != 5 * srk_vgg_tap_workspace_bytes(1);
  for (int mode = 0; mode < 3; ++mode) {
    bad += srk_vgg_tap_plan(1, 2, 2, 64, mode, 1, &items) != 1 || items < 1;
    bad += srk_vgg_tap_plan(2, 34, 38, 64, mode, 1, &items) < 2;
    bad += srk_vgg_tap_plan(16, 512, 512, 64, mode, 1, &items) != slots || srk_vgg_tap_plan(16, 512, 512, 64, mode, 0, &items) != slots;
  }
  bad += srk_vgg_tap_plan(1, 4, 4, 6, SRK_VGG_TAP_POOL, 1, nullptr) != SRK_ERR_BAD_ARG;
  printf(bad ? "vgg_tap_host_check: %d FAILED\n" : "vgg_tap_host_check: ok (%d failures)\n", bad);
  return bad != 0;
}
