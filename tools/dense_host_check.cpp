// A stand-alone run of srk_dense_conv_host (csrc/dense.hip, csrc/dense_common.h) on sliced buffers with guard regions, for
// the host sanitizers: it needs no device and no Python.  Build and run from the repo root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
//         pytorch_super_resolution_model_collection_amd/csrc/dense.hip tools/dense_host_check.cpp -o dense_host_check
//         && ./dense_host_check
// Every buffer is allocated at its exact size: pixel (P - 1) of a slice ends `ld - off - C` floats before the end of its
// buffer and pixel 0 starts `off` floats after its beginning, so a stride or offset mistake is a sanitizer report or a
// changed guard value.  The program checks that every float outside a destination slice keeps its bits, that the NaN
// around the source slices never reaches a result, that beta 0 overwrites NaN and beta 1 adds, the refusals (which come
// before anything is read) and the planner's invariants; the numbers themselves are the CPU suite's business
// (tests/test_dense_cpu.py).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../include/srk.h"

namespace srk {   // dense.hip reports through the library's error slot (csrc/api.hip); this program keeps the last message
static char g_msg[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
}
void note_kernel(const char*, ...) {}
}  // namespace srk

struct Slice {   // `c` channels from channel `off` of a [P][ld] buffer; `guard` everywhere else
  std::vector<float> buf;
  int64_t P;
  int ld, off, c;
  float guard;
  Slice(int64_t P_, int c_, int off_, int tail, float guard_, std::mt19937* gen, float inside = 0.f)
      : buf((size_t)P_ * (off_ + c_ + tail), guard_), P(P_), ld(off_ + c_ + tail), off(off_), c(c_), guard(guard_) {
    std::normal_distribution<float> nd(0.f, 1.f);
    for (int64_t p = 0; p < P; ++p)
      for (int k = 0; k < c; ++k) buf[(size_t)p * ld + off + k] = gen ? nd(*gen) : inside;
  }
  float* ptr() { return buf.data() + off; }
  float at(int64_t p, int k) const { return buf[(size_t)p * ld + off + k]; }
  bool guards_intact() const {
    for (int64_t p = 0; p < P; ++p)
      for (int k = 0; k < ld; ++k)
        if ((k < off || k >= off + c) && memcmp(&buf[(size_t)p * ld + k], &guard, 4)) return false;
    return true;
  }
  bool finite() const {
    for (int64_t p = 0; p < P; ++p)
      for (int k = 0; k < c; ++k)
        if (!isfinite(at(p, k))) return false;
    return true;
  }
};

struct Case {
  const char* name;
  int N, H, W, K, CA, CB, Cout, act, res;
};

static int fail(const Case& c, const char* what) {
  printf("%s: %s (%s)\n", c.name, what, srk::g_msg);
  return 1;
}

static int run(const Case& c) {
  std::mt19937 gen(99u + (unsigned)c.H * 13 + (unsigned)c.CA + (unsigned)c.CB * 3);
  std::normal_distribution<float> nd(0.f, 1.f);
  const int64_t P = (int64_t)c.N * c.H * c.W;
  const int Ctot = c.CA + c.CB;
  const float nanv = NAN;
  Slice A(P, c.CA, 16, 32, nanv, &gen), B(P, c.CB, 32, 16, nanv, &gen), R(P, c.Cout, 16, 0, nanv, &gen);
  Slice DY(P, c.Cout, 48, 16, nanv, &gen), ADD(P, c.CA, 16, 16, nanv, &gen);
  std::vector<float> W((size_t)c.Cout * Ctot * c.K * c.K), bias(c.Cout);
  for (auto& e : W) e = 0.1f * nd(gen);
  for (auto& e : bias) e = 0.1f * nd(gen);
  Slice Y(P, c.Cout, 32, 16, 7.5f, nullptr, nanv);      // the destination: NaN inside, a guard value outside
  srk_dense_desc d;
  memset(&d, 0, sizeof(d));
  d.N = c.N, d.H = c.H, d.W = c.W, d.K = c.K, d.CA = c.CA, d.CB = c.CB, d.Cout = c.Cout;
  d.ldA = A.ld, d.ldB = B.ld, d.ldY = Y.ld, d.ldR = R.ld, d.ldDy = DY.ld, d.ldAdd = ADD.ld;
  d.act = c.act, d.slope = 0.2f, d.terms = 3;
  if (!srk_dense_conv_supported(&d)) return fail(c, "not supported");
  float* Bp = c.CB ? B.ptr() : nullptr;
  if (srk_dense_conv_host(&d, 0, A.ptr(), Bp, W.data(), bias.data(), c.res ? R.ptr() : nullptr, Y.ptr(), nullptr, nullptr,
                          nullptr, 0.f, nullptr, 0.f, nullptr, nullptr, 0.f))
    return fail(c, "forward failed");
  if (!Y.finite() || !Y.guards_intact()) return fail(c, "forward: NaN reached the result or a guard moved");
  // data gradient: beta 0 over NaN with add, then beta 1 (doubles what the convolution contributes)
  Slice DA(P, c.CA, 16, 16, -3.25f, nullptr, nanv), DB(P, c.CB, 48, 16, -3.25f, nullptr, nanv);
  d.ldDA = DA.ld, d.ldDB = DB.ld;
  float* DBp = c.CB ? DB.ptr() : nullptr;
  if (srk_dense_conv_host(&d, 1, nullptr, nullptr, W.data(), nullptr, nullptr, Y.ptr(), DY.ptr(), ADD.ptr(), DA.ptr(), 0.f,
                          DBp, 0.f, nullptr, nullptr, 0.f))
    return fail(c, "backward_data failed");
  if (!DA.finite() || !DB.finite() || !DA.guards_intact() || !DB.guards_intact())
    return fail(c, "backward_data: NaN reached a result or a guard moved");
  Slice DA1 = DA, DB1 = DB;
  if (srk_dense_conv_host(&d, 1, nullptr, nullptr, W.data(), nullptr, nullptr, Y.ptr(), DY.ptr(), nullptr, DA.ptr(), 1.f, DBp,
                          1.f, nullptr, nullptr, 0.f))
    return fail(c, "backward_data (beta 1) failed");
  for (int64_t p = 0; p < P; ++p) {
    for (int k = 0; k < c.CA; ++k) {
      const double conv = (double)DA1.at(p, k) - (double)ADD.at(p, k);
      if (fabs((double)DA.at(p, k) - ((double)DA1.at(p, k) + conv)) > 1e-4 * (1.0 + fabs(conv))) return fail(c, "dA: beta 1 does not add");
    }
    for (int k = 0; k < c.CB; ++k)
      if (fabs((double)DB.at(p, k) - 2.0 * DB1.at(p, k)) > 1e-4 * (1.0 + fabs((double)DB1.at(p, k)))) return fail(c, "dB: beta 1 does not add");
  }
  if (!DA.guards_intact() || !DB.guards_intact()) return fail(c, "backward_data (beta 1): a guard moved");
  // weight gradient: exact-size dW / db, beta 0 over NaN then beta 1
  std::vector<float> dW(W.size(), nanv), db(c.Cout, nanv);
  if (srk_dense_conv_host(&d, 2, A.ptr(), Bp, nullptr, nullptr, nullptr, Y.ptr(), DY.ptr(), nullptr, nullptr, 0.f, nullptr, 0.f,
                          dW.data(), db.data(), 0.f))
    return fail(c, "backward_weight failed");
  std::vector<float> dW1 = dW, db1 = db;
  if (srk_dense_conv_host(&d, 2, A.ptr(), Bp, nullptr, nullptr, nullptr, Y.ptr(), DY.ptr(), nullptr, nullptr, 0.f, nullptr, 0.f,
                          dW.data(), db.data(), 1.f))
    return fail(c, "backward_weight (beta 1) failed");
  for (size_t i = 0; i < dW.size(); ++i)
    if (!isfinite(dW1[i]) || fabs((double)dW[i] - 2.0 * dW1[i]) > 1e-4 * (1.0 + fabs((double)dW1[i]))) return fail(c, "dW: beta");
  for (size_t i = 0; i < db.size(); ++i)
    if (!isfinite(db1[i]) || fabs((double)db[i] - 2.0 * db1[i]) > 1e-4 * (1.0 + fabs((double)db1[i]))) return fail(c, "db: beta");
  // the planner: every pixel in exactly one range, the workspace holds every range
  srk_dense_plan pl;
  pl.struct_size = sizeof(pl);
  if (srk_dense_conv_plan(&d, &pl) || pl.splits < 1 || (int64_t)pl.splits * pl.split_pixels < P ||
      (int64_t)(pl.splits - 1) * pl.split_pixels >= P || pl.ws_bytes < (uint64_t)pl.splits * pl.partial_floats * 4 ||
      pl.ws_bytes != srk_dense_conv_workspace_bytes(&d))
    return fail(c, "planner");
  return 0;
}

int main() {
  const Case table[] = {{"1x1_k1", 2, 1, 1, 1, 16, 0, 16, SRK_ACT_NONE, 0},     {"1x1_k3", 2, 1, 1, 3, 16, 16, 32, SRK_ACT_RELU, 1},
                        {"3x5", 2, 3, 5, 3, 16, 0, 16, SRK_ACT_RELU, 0},        {"3x5_k1", 2, 3, 5, 1, 64, 48, 64, SRK_ACT_NONE, 1},
                        {"3x5_b160", 2, 3, 5, 3, 64, 160, 32, SRK_ACT_LRELU, 0}, {"7x9", 2, 7, 9, 3, 16, 48, 64, SRK_ACT_RELU, 0},
                        {"7x9_lff", 2, 7, 9, 1, 64, 160, 64, SRK_ACT_NONE, 1},   {"17x33", 1, 17, 33, 3, 16, 48, 48, SRK_ACT_LRELU, 1}};
  int bad = 0;
  for (const Case& c : table) bad += run(c);
  // refusals come before any read: the pointers below are never dereferenced
  float one = 0.f;
  srk_dense_desc d;
  memset(&d, 0, sizeof(d));
  d.N = d.H = d.W = 1, d.K = 3, d.CA = 16, d.Cout = 16, d.ldA = d.ldY = 16, d.terms = 3;
  auto fwd = [&]() {
    return srk_dense_conv_host(&d, 0, &one, &one, &one, &one, nullptr, &one, nullptr, nullptr, nullptr, 0.f, nullptr, 0.f,
                               nullptr, nullptr, 0.f);
  };
  d.CA = 24;
  bad += fwd() != SRK_ERR_UNSUPPORTED || !strstr(srk::g_msg, "CA = 24");
  d.CA = 16, d.Cout = 80;
  bad += fwd() != SRK_ERR_UNSUPPORTED || !strstr(srk::g_msg, "Cout = 80");
  d.Cout = 16, d.K = 2;
  bad += fwd() != SRK_ERR_UNSUPPORTED || !strstr(srk::g_msg, "K = 2");
  d.K = 3, d.terms = 5;
  bad += fwd() != SRK_ERR_BAD_ARG;
  d.terms = 3, d.ldA = 8;
  bad += fwd() != SRK_ERR_BAD_ARG;
  d.ldA = 16;
  bad += srk_dense_conv_host(&d, 0, nullptr, nullptr, &one, &one, nullptr, &one, nullptr, nullptr, nullptr, 0.f, nullptr, 0.f,
                             nullptr, nullptr, 0.f) != SRK_ERR_BAD_ARG;
  bad += srk_dense_conv_host(&d, 3, &one, nullptr, &one, &one, nullptr, &one, nullptr, nullptr, nullptr, 0.f, nullptr, 0.f,
                             nullptr, nullptr, 0.f) != SRK_ERR_BAD_ARG;
  printf(bad ? "dense_host_check: %d FAILED\n" : "dense_host_check: ok (%d failures)\n", bad);
  return bad != 0;
}
