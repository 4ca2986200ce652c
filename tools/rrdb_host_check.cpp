// A stand-alone run of the two host twins ESRGAN adds -- srk_dense_conv_host_ex (csrc/dense.hip) on sliced buffers with
// guard regions and srk_ragan_loss_host (csrc/ragan.hip) on exact-size rows -- for the host sanitizers: it needs no device
// and no Python.  Build and run from the repo root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
//         pytorch_super_resolution_model_collection_amd/csrc/dense.hip pytorch_super_resolution_model_collection_amd/csrc/ragan.hip
//         tools/rrdb_host_check.cpp -o rrdb_host_check && ./rrdb_host_check
// Every buffer is allocated at its exact size (see tools/dense_host_check.cpp): a stride or offset mistake in the new
// skips (R1 through desc.ldR, R2 through the epilogue's ldR2) is a sanitizer report or a changed guard value.  Checked
// here: guards, that NaN around the sources never reaches a result, the epilogue's algebra against the plain twin
// (y_ex = s * y_plain + r1 * R1 + r2 * R2; dA_ex = s * dA_plain + a1 * add; dW_ex = s * dW_plain), bit-equality for the
// identity epilogue, the loss's invariants (finite at +-60, the two gradient rows sum to zero, a NULL row is skipped)
// and the refusals.  The numbers against fp64 autograd are the CPU suite's business (tests/test_rrdb_cpu.py,
// tests/test_ragan_cpu.py).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../include/srk.h"

namespace srk {   // the kernels' files report through the library's error slot (csrc/api.hip); this program keeps the last message
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
  int N, H, W, K, CA, CB, Cout, act;
};
struct Epi {
  const char* name;
  float s, r1;
  int has1;
  float r2;
  int has2;
  float a1;
};

static int fail(const Case& c, const Epi& e, const char* what) {
  printf("%s / %s: %s (%s)\n", c.name, e.name, what, srk::g_msg);
  return 1;
}

static bool near(double got, double want) { return fabs(got - want) <= 1e-5 * (1.0 + fabs(want)); }

static int run(const Case& c, const Epi& ep) {
  std::mt19937 gen(7u + (unsigned)c.H * 13 + (unsigned)c.CA + (unsigned)c.CB * 3);
  std::normal_distribution<float> nd(0.f, 1.f);
  const int64_t P = (int64_t)c.N * c.H * c.W;
  const int Ctot = c.CA + c.CB;
  const float nanv = NAN;
  Slice A(P, c.CA, 16, 32, nanv, &gen), B(P, c.CB, 32, 16, nanv, &gen), R1(P, c.Cout, 16, 0, nanv, &gen);
  Slice R2(P, c.Cout, 32, 4, nanv, &gen), DY(P, c.Cout, 48, 16, nanv, &gen), ADD(P, c.CA, 16, 16, nanv, &gen);
  std::vector<float> W((size_t)c.Cout * Ctot * c.K * c.K), bias(c.Cout);
  for (auto& e : W) e = 0.1f * nd(gen);
  for (auto& e : bias) e = 0.1f * nd(gen);
  Slice Y(P, c.Cout, 32, 16, 7.5f, nullptr, nanv), Y0(P, c.Cout, 32, 16, 7.5f, nullptr, nanv);
  srk_dense_desc d;
  memset(&d, 0, sizeof(d));
  d.N = c.N, d.H = c.H, d.W = c.W, d.K = c.K, d.CA = c.CA, d.CB = c.CB, d.Cout = c.Cout;
  d.ldA = A.ld, d.ldB = B.ld, d.ldY = Y.ld, d.ldR = R1.ld, d.ldDy = DY.ld, d.ldAdd = ADD.ld;
  d.act = c.act, d.slope = 0.2f, d.terms = 3;
  srk_dense_epilogue e;
  e.struct_size = sizeof(e), e.s = ep.s, e.r1 = ep.r1, e.r2 = ep.r2, e.ldR2 = R2.ld, e.a1 = ep.a1;
  float* Bp = c.CB ? B.ptr() : nullptr;
  float* r1p = ep.has1 ? R1.ptr() : nullptr;
  float* r2p = ep.has2 ? R2.ptr() : nullptr;
  // forward: the epilogue's algebra on top of the plain twin without a residual
  if (srk_dense_conv_host(&d, 0, A.ptr(), Bp, W.data(), bias.data(), nullptr, Y0.ptr(), nullptr, nullptr, nullptr, 0.f, nullptr,
                          0.f, nullptr, nullptr, 0.f))
    return fail(c, ep, "plain forward failed");
  if (srk_dense_conv_host_ex(&d, 0, A.ptr(), Bp, W.data(), bias.data(), r1p, r2p, &e, Y.ptr(), nullptr, nullptr, nullptr, 0.f,
                             nullptr, 0.f, nullptr, nullptr, 0.f))
    return fail(c, ep, "forward failed");
  if (!Y.finite() || !Y.guards_intact()) return fail(c, ep, "forward: NaN reached the result or a guard moved");
  for (int64_t p = 0; p < P; ++p)
    for (int k = 0; k < c.Cout; ++k) {
      const double want = (double)ep.s * Y0.at(p, k) + (ep.has1 ? (double)ep.r1 * R1.at(p, k) : 0.0) +
                          (ep.has2 ? (double)ep.r2 * R2.at(p, k) : 0.0);
      if (!near(Y.at(p, k), want)) return fail(c, ep, "forward: not s * y + r1 * R1 + r2 * R2");
    }
  // data gradient (the saved output is the activation's own: Y0), beta 0 over NaN
  Slice DA(P, c.CA, 16, 16, -3.25f, nullptr, nanv), DB(P, c.CB, 48, 16, -3.25f, nullptr, nanv);
  Slice DA0(P, c.CA, 16, 16, -3.25f, nullptr, nanv), DB0(P, c.CB, 48, 16, -3.25f, nullptr, nanv);
  d.ldDA = DA.ld, d.ldDB = DB.ld;
  float* DBp = c.CB ? DB.ptr() : nullptr;
  float* DB0p = c.CB ? DB0.ptr() : nullptr;
  if (srk_dense_conv_host(&d, 1, nullptr, nullptr, W.data(), nullptr, nullptr, Y0.ptr(), DY.ptr(), nullptr, DA0.ptr(), 0.f, DB0p,
                          0.f, nullptr, nullptr, 0.f))
    return fail(c, ep, "plain backward_data failed");
  if (srk_dense_conv_host_ex(&d, 1, nullptr, nullptr, W.data(), nullptr, nullptr, nullptr, &e, Y0.ptr(), DY.ptr(), ADD.ptr(),
                             DA.ptr(), 0.f, DBp, 0.f, nullptr, nullptr, 0.f))
    return fail(c, ep, "backward_data failed");
  if (!DA.finite() || !DB.finite() || !DA.guards_intact() || !DB.guards_intact())
    return fail(c, ep, "backward_data: NaN reached a result or a guard moved");
  for (int64_t p = 0; p < P; ++p) {
    for (int k = 0; k < c.CA; ++k)
      if (!near(DA.at(p, k), (double)ep.s * DA0.at(p, k) + (double)ep.a1 * ADD.at(p, k))) return fail(c, ep, "dA: not s * dA + a1 * add");
    for (int k = 0; k < c.CB; ++k)
      if (!near(DB.at(p, k), (double)ep.s * DB0.at(p, k))) return fail(c, ep, "dB: not s * dB");
  }
  // weight gradient
  std::vector<float> dW(W.size(), nanv), db(c.Cout, nanv), dW0(W.size(), nanv), db0(c.Cout, nanv);
  if (srk_dense_conv_host(&d, 2, A.ptr(), Bp, nullptr, nullptr, nullptr, Y0.ptr(), DY.ptr(), nullptr, nullptr, 0.f, nullptr, 0.f,
                          dW0.data(), db0.data(), 0.f))
    return fail(c, ep, "plain backward_weight failed");
  if (srk_dense_conv_host_ex(&d, 2, A.ptr(), Bp, nullptr, nullptr, nullptr, nullptr, &e, Y0.ptr(), DY.ptr(), nullptr, nullptr, 0.f,
                             nullptr, 0.f, dW.data(), db.data(), 0.f))
    return fail(c, ep, "backward_weight failed");
  for (size_t i = 0; i < dW.size(); ++i)
    if (!near(dW[i], (double)ep.s * dW0[i])) return fail(c, ep, "dW: not s * dW");
  for (size_t i = 0; i < db.size(); ++i)
    if (!near(db[i], (double)ep.s * db0[i])) return fail(c, ep, "db: not s * db");
  // the identity epilogue (and no epilogue at all): the plain twin's bits
  if (ep.s == 1.f && ep.r1 == 1.f && !ep.has2) {
    Slice Ya(P, c.Cout, 32, 16, 7.5f, nullptr, nanv), Yb(P, c.Cout, 32, 16, 7.5f, nullptr, nanv);
    if (srk_dense_conv_host(&d, 0, A.ptr(), Bp, W.data(), bias.data(), r1p, Ya.ptr(), nullptr, nullptr, nullptr, 0.f, nullptr, 0.f,
                            nullptr, nullptr, 0.f) ||
        srk_dense_conv_host_ex(&d, 0, A.ptr(), Bp, W.data(), bias.data(), r1p, nullptr, nullptr, Yb.ptr(), nullptr, nullptr,
                               nullptr, 0.f, nullptr, 0.f, nullptr, nullptr, 0.f))
      return fail(c, ep, "identity forward failed");
    if (memcmp(Ya.buf.data(), Yb.buf.data(), Ya.buf.size() * 4) || memcmp(Ya.buf.data(), Y.buf.data(), Ya.buf.size() * 4))
      return fail(c, ep, "identity epilogue: bits differ from the plain twin");
  }
  return 0;
}

static int ragan_case(int B, int mode, bool extreme, bool equal) {
  std::mt19937 gen(31u + (unsigned)B * 7 + (unsigned)mode);
  std::normal_distribution<float> nd(0.f, 2.f);
  std::vector<float> real(B), fake(B);        // exact size: an index past B is a sanitizer report
  for (int i = 0; i < B; ++i) real[i] = nd(gen), fake[i] = equal ? real[i] : nd(gen) - 0.5f;
  if (extreme) {
    real[0] = 60.f, fake[0] = -60.f;
    if (B > 1) real[1] = -60.f, fake[1] = 60.f;
  }
  std::vector<double> dr(B, NAN), df(B, NAN), df2(B, NAN);
  double loss = NAN, loss2 = NAN;
  if (srk_ragan_loss_host(real.data(), fake.data(), B, mode, 1.0, &loss, dr.data(), df.data())) return 1;
  if (srk_ragan_loss_host(real.data(), fake.data(), B, mode, 1.0, &loss2, nullptr, df2.data())) return 1;
  if (!isfinite(loss) || loss < 0.0 || loss != loss2) return 1;
  double sum = 0.0, mag = 0.0;
  for (int i = 0; i < B; ++i) {
    if (!isfinite(dr[i]) || !isfinite(df[i]) || df[i] != df2[i]) return 1;
    sum += dr[i] + df[i], mag += fabs(dr[i]) + fabs(df[i]);
  }
  if (fabs(sum) > 1e-12 * (1.0 + mag)) return 1;     // a shift of every logit leaves the loss alone
  if (B == 1) {                                      // a = r - f: the loss is softplus(-+(r - f))
    const double x = mode ? (double)real[0] - fake[0] : (double)fake[0] - real[0];
    if (fabs(loss - ((x > 0 ? x : 0) + log1p(exp(-fabs(x))))) > 1e-12 * (1.0 + loss)) return 1;
  }
  return 0;
}

int main() {
  const Case table[] = {{"1x1_k3", 2, 1, 1, 3, 16, 16, 32, SRK_ACT_NONE},      {"3x5_k1", 2, 3, 5, 1, 64, 48, 64, SRK_ACT_NONE},
                        {"3x5_growth", 2, 3, 5, 3, 64, 64, 32, SRK_ACT_LRELU}, {"5x7_conv5", 1, 5, 7, 3, 64, 128, 64, SRK_ACT_NONE},
                        {"7x9_conv5", 2, 7, 9, 3, 16, 64, 16, SRK_ACT_NONE},   {"7x9_single", 1, 7, 9, 3, 16, 0, 16, SRK_ACT_LRELU}};
  const Epi epis[] = {{"plain", 1.f, 1.f, 1, 0.f, 0, 1.f},    {"s_only", 0.2f, 1.f, 0, 0.f, 0, 1.f},
                      {"rdb", 0.2f, 1.f, 1, 0.f, 0, 1.f},      {"r2_only", 1.f, 1.f, 0, 0.5f, 1, 0.25f},
                      {"rrdb", 0.04f, 0.2f, 1, 1.f, 1, 0.2f},  {"all_odd", -1.5f, 0.75f, 1, -0.3f, 1, -2.f}};
  int bad = 0;
  for (const Case& c : table)
    for (const Epi& e : epis) bad += run(c, e);
  const int Bs[] = {1, 2, 3, 16, 257};
  for (int B : Bs)
    for (int mode = 0; mode < 2; ++mode) {
      bad += ragan_case(B, mode, false, false);
      bad += ragan_case(B, mode, true, false);
      bad += ragan_case(B, mode, false, true);
    }
  // refusals come before any read: the pointers below are never dereferenced
  float one = 0.f;
  double loss = 0.0;
  bad += srk_ragan_loss_host(&one, &one, 0, 0, 1.0, &loss, nullptr, nullptr) != SRK_ERR_BAD_ARG || !strstr(srk::g_msg, "B = 0");
  bad += srk_ragan_loss_host(nullptr, &one, 1, 0, 1.0, &loss, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  bad += srk_ragan_loss_host(&one, &one, 1, 1, 1.0, nullptr, nullptr, nullptr) != SRK_ERR_BAD_ARG;
  srk_dense_desc d;
  memset(&d, 0, sizeof(d));
  d.N = d.H = d.W = 1, d.K = 3, d.CA = 16, d.Cout = 16, d.ldA = d.ldY = d.ldR = 16, d.terms = 3;
  srk_dense_epilogue e;
  e.struct_size = sizeof(e), e.s = 0.2f, e.r1 = 1.f, e.r2 = 1.f, e.ldR2 = 12, e.a1 = 1.f;
  auto fwd = [&](const srk_dense_epilogue* ep, const float* r2) {
    return srk_dense_conv_host_ex(&d, 0, &one, nullptr, &one, &one, nullptr, r2, ep, &one, nullptr, nullptr, nullptr, 0.f, nullptr,
                                  0.f, nullptr, nullptr, 0.f);
  };
  bad += fwd(&e, &one) != SRK_ERR_BAD_ARG || !strstr(srk::g_msg, "ldR2 = 12");
  bad += fwd(nullptr, &one) != SRK_ERR_BAD_ARG;                 // R2 without its scale and stride
  e.ldR2 = 16, e.s = INFINITY;
  bad += fwd(&e, nullptr) != SRK_ERR_BAD_ARG || !strstr(srk::g_msg, "finite");
  e.s = 0.2f, e.struct_size = 8;
  bad += fwd(&e, nullptr) != SRK_ERR_BAD_ARG || !strstr(srk::g_msg, "struct_size");
  e.struct_size = sizeof(e), d.Cout = 80;
  bad += fwd(&e, nullptr) != SRK_ERR_UNSUPPORTED || !strstr(srk::g_msg, "Cout = 80");
  printf(bad ? "rrdb_host_check: %d FAILED\n" : "rrdb_host_check: ok (%d failures)\n", bad);
  return bad != 0;
}
