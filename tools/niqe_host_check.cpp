// A stand-alone run of srk_niqe_features_host and srk_niqe_tables_host (csrc/niqe.hip, csrc/niqe_common.h) over the
// shapes of the tests' case table, for the host sanitizers: it needs no device and no Python.  Build and run from the
// repo root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
//         pytorch_super_resolution_model_collection_amd/csrc/niqe.hip tools/niqe_host_check.cpp -o niqe_host_check && ./niqe_host_check
// Every buffer is allocated at its exact size (the picture as the strided view's own extent), so a read or write past
// any of them is a report.  The program also checks the refusals (which must come before anything is read), that float
// and byte pictures of the same bytes give the same bits through every layout, that a flat picture gives NaN features and
// zero sharpness, and that the table search agrees with a linear argmin; the numbers themselves are the CPU suite's
// business (tests/test_niqe_cpu.py).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../include/srk.h"

namespace srk {   // niqe.hip reports through the library's error slot (csrc/api.hip); this program keeps the last message
static char g_msg[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
}
}  // namespace srk

struct Case {
  int C, H, W, block, shave;
};

static std::vector<double> g_tables;

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

static int run(const Case& c) {
  std::mt19937 gen(99u + (unsigned)c.H * 131 + (unsigned)c.W);
  std::uniform_int_distribution<int> byte(0, 255);
  const size_t plane = (size_t)c.H * c.W;
  std::vector<uint8_t> u8(plane * c.C);
  for (size_t i = 0; i < plane; ++i) {   // smooth-ish rows plus noise: both signs in every map
    const int base = 40 + (int)((i % c.W) * 150 / c.W);
    for (int ch = 0; ch < c.C; ++ch) u8[ch * plane + i] = (uint8_t)((base + byte(gen) / 3) & 255);
  }
  const int nh = (c.H - 2 * c.shave) / c.block, nw = (c.W - 2 * c.shave) / c.block, blocks = nh * nw;
  std::vector<double> f_u8((size_t)blocks * SRK_NIQE_FEATURES), sharp(blocks), f_f32(f_u8.size()), f_hwc(f_u8.size());
  if (srk_niqe_features_host(u8.data(), 1, nullptr, c.C, c.H, c.W, c.shave, c.block, g_tables.data(), f_u8.data(),
                             sharp.data())) {
    printf("FAIL [%d,%d,%d] block %d: %s\n", c.C, c.H, c.W, c.block, srk::g_msg);
    return 1;
  }
  std::vector<float> f32(u8.size()), hwc(u8.size());
  for (size_t i = 0; i < u8.size(); ++i) f32[i] = (float)u8[i] / 255.0f;
  for (int ch = 0; ch < c.C; ++ch)
    for (size_t i = 0; i < plane; ++i) hwc[i * c.C + ch] = f32[ch * plane + i];
  const int64_t chw[3] = {(int64_t)plane, c.W, 1}, last[3] = {1, (int64_t)c.W * c.C, c.C};
  int bad = 0;
  bad |= srk_niqe_features_host(f32.data(), 0, chw, c.C, c.H, c.W, c.shave, c.block, g_tables.data(), f_f32.data(), nullptr);
  bad |= srk_niqe_features_host(hwc.data(), 0, last, c.C, c.H, c.W, c.shave, c.block, g_tables.data(), f_hwc.data(), nullptr);
  if (bad || !same_bits(f_u8, f_f32) || !same_bits(f_u8, f_hwc)) {
    printf("FAIL [%d,%d,%d] block %d: layouts differ (%s)\n", c.C, c.H, c.W, c.block, srk::g_msg);
    return 1;
  }
  int nans = 0;
  for (double v : f_u8) nans += v != v;
  for (double v : sharp)
    if (!(v > 0.0)) {
      printf("FAIL [%d,%d,%d]: sharpness %g\n", c.C, c.H, c.W, v);
      return 1;
    }
  printf("ok   [%d,%d,%d] block %d shave %d: %d blocks, %d NaN features\n", c.C, c.H, c.W, c.block, c.shave, blocks, nans);
  return 0;
}

static int refusals() {
  std::vector<uint8_t> img(3 * 64 * 64);
  std::vector<double> f(16 * SRK_NIQE_FEATURES);
  struct {
    int C, H, W, shave, block;
    const char* want;
  } bad[] = {{3, 64, 64, 0, 15, "got 15"},     {3, 64, 64, 0, 98, "got 98"},         {3, 64, 64, 0, 6, "got 6"},
             {2, 64, 64, 0, 16, "got 2"},      {3, 40, 31, 0, 24, "1 x 1 blocks"},   {3, 64, 64, 20, 24, "1 x 1 blocks"},
             {3, 64, 64, -1, 16, "negative"},  {3, 0, 64, 0, 16, "bad dims"}};
  int fails = 0;
  for (auto& b : bad) {
    srk::g_msg[0] = 0;
    const int rc = srk_niqe_features_host(img.data(), 1, nullptr, b.C, b.H, b.W, b.shave, b.block, g_tables.data(), f.data(),
                                          nullptr);
    if (rc != SRK_ERR_BAD_ARG || !strstr(srk::g_msg, b.want)) {
      printf("FAIL refusal (%d,%d,%d,%d,%d): rc %d, '%s'\n", b.C, b.H, b.W, b.shave, b.block, rc, srk::g_msg);
      ++fails;
    }
  }
  if (srk_niqe_features_host(nullptr, 1, nullptr, 3, 64, 64, 0, 16, g_tables.data(), f.data(), nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_niqe_features_host(img.data(), 1, nullptr, 3, 64, 64, 0, 16, nullptr, f.data(), nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_niqe_features_host(img.data(), 1, nullptr, 3, 64, 64, 0, 16, g_tables.data(), nullptr, nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_niqe_tables_host(nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_niqe_workspace_bytes(197, 99, 96) != (size_t)2 * 48 * 48 * 8 || srk_niqe_workspace_bytes(64, 64, 15) != 0) ++fails;
  printf("%s refusals\n", fails ? "FAIL" : "ok  ");
  return fails;
}

static int flat() {
  std::vector<uint8_t> img(3 * 32 * 48, 88);   // luma 92: the separable sums return it exactly (tests/niqe_ref.py)
  std::vector<double> f(6 * SRK_NIQE_FEATURES), s(6);
  if (srk_niqe_features_host(img.data(), 1, nullptr, 3, 32, 48, 0, 16, g_tables.data(), f.data(), s.data())) return 1;
  int fails = 0;
  for (double v : f) fails += v == v;
  for (double v : s) fails += v != 0.0;
  printf("%s flat picture: NaN features, zero sharpness\n", fails ? "FAIL" : "ok  ");
  return fails;
}

int main() {
  g_tables.resize((size_t)3 * SRK_NIQE_TABLE);
  if (srk_niqe_tables_host(g_tables.data())) return 1;
  int fails = 0;
  for (int j = 1; j < SRK_NIQE_TABLE; ++j) fails += !(g_tables[j] > g_tables[j - 1]);   // what the bisection stands on
  printf("%s r_gam increases\n", fails ? "FAIL" : "ok  ");
  const Case cases[] = {{3, 32, 32, 16, 0}, {3, 50, 70, 16, 0}, {1, 40, 56, 8, 0}, {3, 197, 99, 96, 0},
                        {3, 70, 50, 24, 3}, {1, 16, 130, 16, 0}};
  for (const Case& c : cases) fails += run(c);
  fails += refusals();
  fails += flat();
  printf(fails ? "%d FAILED\n" : "all ok\n", fails);
  return fails ? 1 : 0;
}
