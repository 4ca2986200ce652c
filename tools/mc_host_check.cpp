// A stand-alone run of srk_motion_fuse_host, srk_flow_warp_host and srk_flow_huber_host (csrc/mc.hip, csrc/mc_common.h)
// over the shapes of the tests' table, for the host sanitizers: it needs no device and no Python.  Build and run from the
// repo root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
//         pytorch_super_resolution_model_collection_amd/csrc/mc.hip tools/mc_host_check.cpp -o mc_host_check && ./mc_host_check
// Every buffer is allocated at its exact size, so a corner read or a store past a plane is a report.  The flows are the
// hard ones: far outside the picture on every side, exactly on the bounds, NaN and infinities.  The program also checks
// that both flow layouts give the same bits, that a zero flow copies the frames, that a constant flow is perfectly smooth,
// and the refusals (which must come before anything is read); the numbers themselves are the CPU suite's business
// (tests/test_mc_cpu.py).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <random>
#include <vector>

#include "../include/srk.h"
#include "../include/srk_mc.h"

namespace srk {   // mc.hip reports through the library's error slot (csrc/api.hip); this program keeps the last message
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

static int run(const Case& c) {
  std::mt19937 gen(5u + (unsigned)c.W * 131 + (unsigned)c.H * 7 + (unsigned)c.N);
  std::uniform_real_distribution<float> unit(0.f, 1.f), wide(-2.5f, 2.5f);
  const size_t hw = (size_t)c.H * c.W, rows = 2 * (size_t)c.N;
  std::vector<float> frames((size_t)c.N * 3 * c.C * hw), flow(rows * 2 * hw), last(rows * 2 * hw);
  for (float& v : frames) v = unit(gen);
  const float special[] = {0.f, -1.f, 1.f, -1e9f, 1e9f, std::numeric_limits<float>::quiet_NaN(),
                           std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), 0.25f};
  for (size_t i = 0; i < flow.size(); ++i)
    flow[i] = i % 3 == 0 ? special[(i / 3) % 9] : wide(gen) * (float)(c.W > c.H ? c.W : c.H);
  for (size_t r = 0; r < rows; ++r)
    for (int k = 0; k < 2; ++k)
      for (size_t p = 0; p < hw; ++p) last[(r * hw + p) * 2 + k] = flow[(r * 2 + k) * hw + p];
  const int64_t nchw[4] = {(int64_t)(2 * hw), (int64_t)hw, c.W, 1}, nhwc[4] = {(int64_t)(2 * hw), 1, 2 * (int64_t)c.W, 2};
  std::vector<double> g((size_t)c.N * 3 * c.C * hw);
  for (double& v : g) v = wide(gen);
  int fails = 0;
  std::vector<double> fused(g.size()), fused2(g.size()), d(flow.size()), d2(flow.size());
  double mc = 0, mc2 = 0;
  int bad = srk_motion_fuse_host(frames.data(), flow.data(), nchw, c.N, c.C, c.H, c.W, 0.5, g.data(), fused.data(), &mc, d.data());
  bad |= srk_motion_fuse_host(frames.data(), last.data(), nhwc, c.N, c.C, c.H, c.W, 0.5, g.data(), fused2.data(), &mc2, d2.data());
  bad |= srk_motion_fuse_host(frames.data(), flow.data(), nchw, c.N, c.C, c.H, c.W, 1.0, nullptr, fused2.data(), &mc2, nullptr);
  if (bad) {
    printf("FAIL motion_fuse %d %d %d %d: %s\n", c.N, c.C, c.H, c.W, srk::g_msg);
    return 1;
  }
  fails += memcmp(fused.data(), fused2.data(), fused.size() * sizeof(double)) != 0 || mc != mc2;
  srk_motion_fuse_host(frames.data(), last.data(), nhwc, c.N, c.C, c.H, c.W, 0.5, g.data(), fused2.data(), &mc2, d2.data());
  fails += memcmp(d.data(), d2.data(), d.size() * sizeof(double)) != 0;
  for (double v : fused) fails += !(v >= 0.0 && v <= 1.0);         // a convex combination of pixels, whatever the flow
  for (double v : d) fails += !isfinite(v);
  // the plain warp of the first neighbour through a strided view of the frames
  const int64_t img[4] = {(int64_t)(3 * c.C * hw), (int64_t)hw, c.W, 1};
  std::vector<double> out((size_t)c.N * c.C * hw), dw((size_t)c.N * 2 * hw);
  if (srk_flow_warp_host(frames.data(), img, flow.data(), nchw, c.N, c.C, c.H, c.W, g.data(), out.data(), dw.data())) return 1;
  for (int n = 0; n < c.N; ++n)
    for (size_t i = 0; i < c.C * hw; ++i) fails += out[n * c.C * hw + i] != fused[(size_t)n * 3 * c.C * hw + i];
  // zero flow: the frames themselves, gradient of the fusion alone
  std::fill(flow.begin(), flow.end(), 0.f);
  if (srk_motion_fuse_host(frames.data(), flow.data(), nchw, c.N, c.C, c.H, c.W, 1.0, nullptr, fused.data(), &mc, nullptr)) return 1;
  for (size_t i = 0; i < fused.size(); ++i) fails += fused[i] != (double)frames[i];
  // the smoothness term: both layouts, then a constant flow
  double l1 = 0, l2 = 0;
  for (size_t i = 0; i < flow.size(); ++i) flow[i] = wide(gen);
  for (size_t r = 0; r < rows; ++r)
    for (int k = 0; k < 2; ++k)
      for (size_t p = 0; p < hw; ++p) last[(r * hw + p) * 2 + k] = flow[(r * 2 + k) * hw + p];
  bad = srk_flow_huber_host(flow.data(), nchw, (int)rows, c.H, c.W, 0.01, 1.0, &l1, d.data());
  bad |= srk_flow_huber_host(last.data(), nhwc, (int)rows, c.H, c.W, 0.01, 1.0, &l2, d2.data());
  bad |= srk_flow_huber_host(last.data(), nhwc, (int)rows, c.H, c.W, 0.01, 1.0, &l2, nullptr);
  if (bad) {
    printf("FAIL flow_huber %d %d %d: %s\n", (int)rows, c.H, c.W, srk::g_msg);
    return 1;
  }
  fails += l1 != l2 || memcmp(d.data(), d2.data(), d.size() * sizeof(double)) != 0;
  std::fill(flow.begin(), flow.end(), -3.5f);
  if (srk_flow_huber_host(flow.data(), nchw, (int)rows, c.H, c.W, 0.01, 1.0, &l1, d.data())) return 1;
  fails += fabs(l1 - 0.1) > 1e-12;   // (a sum of M H W equal terms)
  for (double v : d) fails += v != 0.0;
  printf("%s N %d C %d %2d x %2d\n", fails ? "FAIL" : "ok  ", c.N, c.C, c.H, c.W);
  return fails;
}

static int refusals() {
  std::vector<float> frames(2 * 3 * 3 * 12), flow(4 * 2 * 12);
  std::vector<double> out(2 * 9 * 12), d(4 * 2 * 12);
  double loss;
  const int64_t st[4] = {24, 12, 4, 1}, neg[4] = {24, 12, -4, 1}, img[4] = {108, 12, 4, 1};
  struct {
    int N, C, H, W;
    const int64_t* fs;
    const char* want;
  } bad[] = {{0, 3, 3, 4, st, "non-positive size"}, {2, 0, 3, 4, st, "non-positive size"}, {2, 3, 0, 4, st, "non-positive size"},
             {2, 3, 3, 0, st, "non-positive size"}, {2, 3, 3, 4, neg, "negative flow stride"}};
  int fails = 0;
  for (auto& b : bad) {
    srk::g_msg[0] = 0;
    int rc = srk_motion_fuse_host(frames.data(), flow.data(), b.fs, b.N, b.C, b.H, b.W, 1.0, nullptr, out.data(), &loss, d.data());
    if (rc != SRK_ERR_BAD_ARG || !strstr(srk::g_msg, b.want)) {
      printf("FAIL motion_fuse refusal '%s': rc %d, '%s'\n", b.want, rc, srk::g_msg);
      ++fails;
    }
    srk::g_msg[0] = 0;
    rc = srk_flow_warp_host(frames.data(), img, flow.data(), b.fs, b.N, b.C, b.H, b.W, nullptr, out.data(), d.data());
    if (rc != SRK_ERR_BAD_ARG || !strstr(srk::g_msg, b.want)) {
      printf("FAIL flow_warp refusal '%s': rc %d, '%s'\n", b.want, rc, srk::g_msg);
      ++fails;
    }
  }
  if (srk_motion_fuse_host(nullptr, flow.data(), st, 2, 3, 3, 4, 1.0, nullptr, out.data(), &loss, nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_motion_fuse_host(frames.data(), nullptr, st, 2, 3, 3, 4, 1.0, nullptr, out.data(), &loss, nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_motion_fuse_host(frames.data(), flow.data(), nullptr, 2, 3, 3, 4, 1.0, nullptr, out.data(), &loss, nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_motion_fuse_host(frames.data(), flow.data(), st, 2, 3, 3, 4, 1.0, nullptr, nullptr, &loss, nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_motion_fuse_host(frames.data(), flow.data(), st, 2, 3, 3, 4, 1.0, nullptr, out.data(), nullptr, nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_flow_warp_host(frames.data(), neg, flow.data(), st, 2, 3, 3, 4, nullptr, out.data(), nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_flow_warp_host(frames.data(), nullptr, flow.data(), st, 2, 3, 3, 4, nullptr, out.data(), nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_flow_huber_host(flow.data(), st, 4, 3, 4, 0.0, 1.0, &loss, nullptr) != SRK_ERR_BAD_ARG || !strstr(srk::g_msg, "eps")) ++fails;
  if (srk_flow_huber_host(flow.data(), neg, 4, 3, 4, 0.01, 1.0, &loss, nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_flow_huber_host(nullptr, st, 4, 3, 4, 0.01, 1.0, &loss, nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_flow_huber_host(flow.data(), st, 4, 3, 4, 0.01, 1.0, nullptr, nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_flow_huber_host(flow.data(), st, 0, 3, 4, 0.01, 1.0, &loss, nullptr) != SRK_ERR_BAD_ARG) ++fails;
  printf("%s refusals\n", fails ? "FAIL" : "ok  ");
  return fails;
}

int main() {
  const Case cases[] = {{1, 1, 1, 1}, {2, 1, 1, 5}, {2, 3, 5, 1}, {1, 1, 4, 4}, {2, 3, 7, 9}, {1, 1, 17, 70}, {3, 3, 32, 32}};
  int fails = 0;
  for (const Case& c : cases) fails += run(c);
  fails += refusals();
  printf(fails ? "%d FAILED\n" : "all ok\n", fails);
  return fails ? 1 : 0;
}
