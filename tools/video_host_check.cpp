// A stand-alone run of srk_yuv_unpack_host and srk_yuv_pack_host (csrc/video.hip, csrc/video_common.h) over the frame
// sizes of the tests' table, for the host sanitizers: it needs no device and no Python.  Build and run from the repo root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer
//         pytorch_super_resolution_model_collection_amd/csrc/video.hip tools/video_host_check.cpp -o video_host_check && ./video_host_check
// Every buffer is allocated at its exact size and the frames start one byte into theirs, so a read or write past a plane,
// a frame or a batch is a report.  The program also checks the refusals (which must come before anything is read), that
// a Y model's front and tail are inverse to each other, that a channels-last output packs to the same bytes, that bytes
// between and behind the frames are left alone, and the shrink's closed form on every quad of two values; the numbers
// themselves are the CPU suite's business (tests/test_video_cpu.py).
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <random>
#include <vector>

#include "../include/srk.h"

namespace srk {   // video.hip reports through the library's error slot (csrc/api.hip); this program keeps the last message
static char g_msg[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
}
}  // namespace srk

struct Case {
  int W, H, sub;
};

static size_t chroma_pixels(const Case& c, int& cw, int& ch) {
  cw = c.sub == SRK_YUV_420 ? c.W / 2 : (c.sub == SRK_YUV_444 ? c.W : 0);
  ch = c.sub == SRK_YUV_420 ? c.H / 2 : (c.sub == SRK_YUV_444 ? c.H : 0);
  return (size_t)cw * ch;
}

static int run(const Case& c, int N) {
  std::mt19937 gen(7u + (unsigned)c.W * 131 + (unsigned)c.H + (unsigned)N);
  std::uniform_int_distribution<int> byte(0, 255);
  std::uniform_real_distribution<float> unit(-0.25f, 1.25f);
  int cw, ch;
  const size_t ypix = (size_t)c.W * c.H, cpix = chroma_pixels(c, cw, ch), fb = ypix + 2 * cpix, stride = fb + 3;
  const size_t span = (size_t)(N - 1) * stride + fb;
  std::vector<uint8_t> in(1 + span), full(2 * N * ypix), chroma(2 * N * cpix);
  for (auto& b : in) b = (uint8_t)byte(gen);
  for (auto& b : full) b = (uint8_t)byte(gen);
  int fails = 0;
  for (int C = 1; C <= 3; C += 2) {
    std::vector<float> x((size_t)N * C * ypix);
    if (srk_yuv_unpack_host(in.data() + 1, (int64_t)stride, N, c.H, c.W, c.sub, C, c.sub == SRK_YUV_420 ? full.data() : nullptr,
                            x.data())) {
      printf("FAIL unpack %dx%d sub %d C %d: %s\n", c.W, c.H, c.sub, C, srk::g_msg);
      return 1;
    }
    for (float v : x) fails += !(v >= 0.f && v <= 1.f);
    // the tail: the front's own output (a Y model: the identity on Y), then values off the unit interval and NaN
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 1)
        for (size_t i = 0; i < x.size(); ++i)
          x[i] = i % 11 == 0 ? std::numeric_limits<float>::quiet_NaN() : (i % 3 == 0 ? (float)byte(gen) / 255.0f : unit(gen));
      for (int n = 0; n < N && cpix; ++n)
        for (int k = 0; k < 2; ++k)
          memcpy(&chroma[((size_t)k * N + n) * cpix], in.data() + 1 + n * stride + ypix + k * cpix, cpix);
      std::vector<uint8_t> out(1 + span, 0xA5), out_last(1 + span, 0xA5);
      const int64_t nchw[4] = {(int64_t)(C * ypix), (int64_t)ypix, c.W, 1};
      const int64_t nhwc[4] = {(int64_t)(C * ypix), 1, (int64_t)c.W * C, C};
      std::vector<float> last(x.size());
      for (int n = 0; n < N; ++n)
        for (int k = 0; k < C; ++k)
          for (size_t p = 0; p < ypix; ++p) last[(n * ypix + p) * C + k] = x[(n * C + k) * ypix + p];
      int bad = srk_yuv_pack_host(x.data(), nchw, N, C, c.H, c.W, c.sub, C == 1 && cpix ? chroma.data() : nullptr, out.data() + 1,
                                  (int64_t)stride);
      bad |= srk_yuv_pack_host(last.data(), nhwc, N, C, c.H, c.W, c.sub, C == 1 && cpix ? chroma.data() : nullptr,
                               out_last.data() + 1, (int64_t)stride);
      if (bad || out != out_last) {
        printf("FAIL pack %dx%d sub %d C %d pass %d: %s\n", c.W, c.H, c.sub, C, pass, bad ? srk::g_msg : "layouts differ");
        return 1;
      }
      fails += out[0] != 0xA5;
      for (int n = 0; n + 1 < N; ++n)
        for (size_t g = fb; g < stride; ++g) fails += out[1 + n * stride + g] != 0xA5;   // the gap between frames
      if (C == 1 && pass == 0)
        for (int n = 0; n < N; ++n) fails += memcmp(out.data() + 1 + n * stride, in.data() + 1 + n * stride, fb) != 0;
    }
  }
  printf("%s %2d x %2d sub %d N %d\n", fails ? "FAIL" : "ok  ", c.W, c.H, c.sub, N);
  return fails;
}

static int shrink() {
  // a grey gives Cb = Cr = 128 whatever its level, so the quad a b / c d is driven through Cb with the blues (0, 0, 3 k):
  // every quad made of two of their Cb values, the odd one in every position
  int fails = 0;
  std::vector<int> cbs;
  for (int b = 0; b < 256; b += 3) {
    float px[3] = {0.f, 0.f, (float)b / 255.0f};
    const int64_t st[4] = {3, 1, 0, 0};
    uint8_t f[3];
    if (srk_yuv_pack_host(px, st, 1, 3, 1, 1, SRK_YUV_444, nullptr, f, 3)) return 1;
    cbs.push_back(f[1]);
  }
  for (size_t i = 0; i < cbs.size(); ++i)
    for (size_t j = 0; j < cbs.size(); ++j)
      for (int pos = 0; pos < 4; ++pos) {
        float x[12] = {0};
        int q[4];
        for (int k = 0; k < 4; ++k) {
          const bool other = k == pos;
          x[8 + k] = (float)(3 * (other ? j : i)) / 255.0f;
          q[k] = cbs[other ? j : i];
        }
        const int64_t st[4] = {12, 4, 2, 1};
        uint8_t f[6];
        if (srk_yuv_pack_host(x, st, 1, 3, 2, 2, SRK_YUV_420, nullptr, f, 6)) return 1;
        const int want = (((q[0] + q[1] + 1) >> 1) + ((q[2] + q[3] + 1) >> 1) + 1) >> 1;
        fails += f[4] != want;
      }
  printf("%s shrink: rounded after each pass\n", fails ? "FAIL" : "ok  ");
  return fails;
}

static int refusals() {
  std::vector<uint8_t> frames(2 * 36), full(2 * 2 * 24);
  std::vector<float> x(2 * 3 * 24);
  const int64_t st[4] = {72, 24, 6, 1}, neg[4] = {72, 24, -6, 1};
  struct {
    int N, H, W, sub, C;
    int64_t stride;
    const char* want;
  } bad[] = {{0, 4, 6, 0, 3, 36, "non-positive"}, {2, 0, 6, 0, 3, 36, "non-positive"}, {2, 4, 6, 3, 3, 36, "subsampling code 3"},
             {2, 4, 6, 0, 2, 36, "got 2"},        {2, 5, 6, 0, 3, 36, "odd size"},     {2, 4, 7, 0, 1, 36, "odd size"},
             {2, 4, 6, 0, 3, 35, "frame stride 35"}};
  int fails = 0;
  for (auto& b : bad) {
    srk::g_msg[0] = 0;
    int rc = srk_yuv_unpack_host(frames.data(), b.stride, b.N, b.H, b.W, b.sub, b.C, full.data(), x.data());
    if (rc != SRK_ERR_BAD_ARG || !strstr(srk::g_msg, b.want)) {
      printf("FAIL unpack refusal '%s': rc %d, '%s'\n", b.want, rc, srk::g_msg);
      ++fails;
    }
    srk::g_msg[0] = 0;
    rc = srk_yuv_pack_host(x.data(), st, b.N, b.C, b.H, b.W, b.sub, full.data(), frames.data(), b.stride);
    if (rc != SRK_ERR_BAD_ARG || !strstr(srk::g_msg, b.want)) {
      printf("FAIL pack refusal '%s': rc %d, '%s'\n", b.want, rc, srk::g_msg);
      ++fails;
    }
  }
  if (srk_yuv_unpack_host(nullptr, 36, 2, 4, 6, 0, 3, full.data(), x.data()) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_yuv_unpack_host(frames.data(), 36, 2, 4, 6, 0, 3, full.data(), nullptr) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_yuv_unpack_host(frames.data(), 36, 2, 4, 6, 0, 3, nullptr, x.data()) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_yuv_pack_host(nullptr, st, 2, 3, 4, 6, 0, nullptr, frames.data(), 36) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_yuv_pack_host(x.data(), nullptr, 2, 3, 4, 6, 0, nullptr, frames.data(), 36) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_yuv_pack_host(x.data(), st, 2, 3, 4, 6, 0, nullptr, nullptr, 36) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_yuv_pack_host(x.data(), neg, 2, 3, 4, 6, 0, nullptr, frames.data(), 36) != SRK_ERR_BAD_ARG) ++fails;
  if (srk_yuv_pack_host(x.data(), st, 2, 1, 4, 6, 0, nullptr, frames.data(), 36) != SRK_ERR_BAD_ARG) ++fails;
  printf("%s refusals\n", fails ? "FAIL" : "ok  ");
  return fails;
}

int main() {
  const Case cases[] = {{2, 2, SRK_YUV_420}, {6, 4, SRK_YUV_420}, {34, 22, SRK_YUV_420}, {64, 48, SRK_YUV_420},
                        {7, 5, SRK_YUV_444}, {5, 3, SRK_YUV_MONO}};
  int fails = 0;
  for (const Case& c : cases)
    for (int N : {1, 3}) fails += run(c, N);
  fails += shrink();
  fails += refusals();
  printf(fails ? "%d FAILED\n" : "all ok\n", fails);
  return fails ? 1 : 0;
}
