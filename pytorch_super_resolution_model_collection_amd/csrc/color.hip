// The colour tail of test_single / test (edsr.py:276-322, utils.py:116-131) on the GPU, bit-exact with Pillow.
//
// The reference opens a picture, converts RGB -> YCbCr with Pillow, super-resolves the Y plane, resizes Cb and Cr with
// Pillow's bicubic, merges and converts back, and quantises the net's float output with ToPILImage after clamp(0, 1).
// Pillow's conversions (src/libImaging/ConvertYCbCr.c, SCALE = 6) are integer table look-ups.  Their closed form:
//     T(c, i) = (int)(c * 64 * i + 0.5)                 C cast: truncation toward zero, i = 0..255
//     Y  = (T(.299, r) + T(.587, g) + T(.114, b)) >> 6
//     Cb = ((T(-.16874, r) + T(-.33126, g) + 32 b) >> 6) + 128                    >> is arithmetic
//     Cr = ((32 r + T(-.41869, g) + T(-.08131, b)) >> 6) + 128
//     U(c, i) = (int)(c * 64 * (i - 128) + 0.5)
//     R = clip8(y + (U(1.402, cr) >> 6))
//     G = clip8(y + ((U(-.34414, cb) + U(-.71414, cr)) >> 6))
//     B = clip8(y + (U(1.772, cb) >> 6))
// (checked against Pillow for all 2^24 inputs in both directions by tests/test_color_cpu.py; the six-digit BT.601
// coefficients do NOT reproduce Pillow).  The tables are built ONCE, in IEEE double by the compiler's constant evaluator
// (make_color_tables is constexpr: no run-time initialisation, no per-device state, nothing to upload), and the same
// object is what the host helpers read and what the kernels get as a __constant__; a kernel copies the tables it needs
// into LDS and looks them up per pixel -- the floating-point expression is never evaluated on the device.
//
// These are byte-stream kernels: a thread handles a run of 16 pixels of one row, so an interleaved RGB run is 48 bytes =
// three 16-byte accesses, an 8-bit plane run one, a float plane run four.  Every access of a run is 16-byte wide when
// its address is 16-byte aligned and the run is complete, else it falls back to scalar accesses (row tails, odd widths,
// unaligned row strides) -- decided per pointer, so an unaligned source does not cost the stores their width.  The
// launchers hand a dense image over as ONE row (flatten_rows), so that an odd width does not misalign every other row.
#include "color_common.h"   // the tables, quant_u8, the run accessors and the run writer (shared with tile.hip)

namespace srk {

// interleaved 8-bit RGB [H][W][3] (row stride in bytes) -> any of: Y as fp32 Y / 255 (ToTensor), Y as 8-bit, Cb and Cr
// as 8-bit planar [2][H][W].  One pass; a NULL output is skipped.
__global__ __launch_bounds__(256) void k_rgb_to_ycc(const unsigned char* __restrict__ rgb, long long row_stride, int H, int W,
                                                    float* __restrict__ y_f32, unsigned char* __restrict__ y_u8,
                                                    unsigned char* __restrict__ cbcr) {
  __shared__ alignas(16) int16_t tab[kFwdTabs * 256];
  stage_tables<kFwdTabs>(kColorDev.fwd, tab);
  const size_t chunks = (size_t)(W + kRun - 1) / kRun;
  const size_t items = chunks * (size_t)H;
  const size_t plane = (size_t)H * W;
  for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
    const size_t row = it / chunks;
    const int x0 = (int)(it % chunks) * kRun;
    const int n = W - x0 < kRun ? W - x0 : kRun;
    const bool full = n == kRun;
    const unsigned char* src = rgb + (long long)row * row_stride + (long long)x0 * 3;
    unsigned w[12];
    load_bytes<12>(src, full && aligned16(src), n * 3, w);
    unsigned yw[4] = {0, 0, 0, 0}, bw[4] = {0, 0, 0, 0}, rw[4] = {0, 0, 0, 0};
    float yf[kRun];
#pragma unroll
    for (int p = 0; p < kRun; ++p) {
      int y, cb, cr;
      rgb_to_ycc_px(tab, (int)get_byte(w, 3 * p), (int)get_byte(w, 3 * p + 1), (int)get_byte(w, 3 * p + 2), y, cb, cr);
      yw[p >> 2] |= (unsigned)y << ((p & 3) * 8);
      bw[p >> 2] |= (unsigned)cb << ((p & 3) * 8);
      rw[p >> 2] |= (unsigned)cr << ((p & 3) * 8);
      yf[p] = (float)y / 255.0f;
    }
    const size_t o = row * (size_t)W + x0;
    if (y_u8) store_bytes<4>(y_u8 + o, full && aligned16(y_u8 + o), n, yw);
    if (cbcr) {
      store_bytes<4>(cbcr + o, full && aligned16(cbcr + o), n, bw);
      store_bytes<4>(cbcr + plane + o, full && aligned16(cbcr + plane + o), n, rw);
    }
    if (y_f32) {
      float* d = y_f32 + o;
      if (full && aligned16(d)) {
#pragma unroll
        for (int q = 0; q < kRun / 4; ++q)
          reinterpret_cast<float4*>(d)[q] = make_float4(yf[4 * q], yf[4 * q + 1], yf[4 * q + 2], yf[4 * q + 3]);
      } else {
#pragma unroll
        for (int p = 0; p < kRun; ++p)
          if (p < n) d[p] = yf[p];
      }
    }
  }
}

// fp32 [C][H][W] through element strides -> interleaved 8-bit [H][W][C], quantised like ToPILImage after clamp(0, 1).
// The nets hand back channels-last tensors (sc = 1, sw = C): for C = 3 a run is then 48 consecutive floats.
template <int C>
__global__ __launch_bounds__(256) void k_to_u8(const float* __restrict__ x, Strides4 s, unsigned char* __restrict__ out, int H,
                                               int W) {
  const size_t chunks = (size_t)(W + kRun - 1) / kRun;
  const size_t items = chunks * (size_t)H;
  const PicDst dst{nullptr, out, nullptr, nullptr};
  for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
    const size_t row = it / chunks;
    const int x0 = (int)(it % chunks) * kRun;
    const int n = W - x0 < kRun ? W - x0 : kRun;
    float v[C][kRun];
    load_run<C>(x + (long long)row * s.h + (long long)x0 * s.w, s.c, s.w, n, v);
    store_run<C, kDstU8>(v, run_mask(n), n, row * (size_t)W + x0, 0, dst, nullptr);
  }
}

// Fused tail of the Y models: Y (fp32 through element strides, quantised as in k_to_u8 -- the quantised plane never goes
// to memory -- or an 8-bit plane) + 8-bit Cb / Cr planes -> interleaved 8-bit RGB [H][W][3].
__global__ __launch_bounds__(256) void k_ycc_to_rgb(const float* __restrict__ y_f32, long long y_sh, long long y_sw,
                                                    const unsigned char* __restrict__ y_u8,
                                                    const unsigned char* __restrict__ cb,
                                                    const unsigned char* __restrict__ cr, unsigned char* __restrict__ rgb,
                                                    int H, int W) {
  __shared__ alignas(16) int16_t tab[kInvTabs * 256];
  stage_tables<kInvTabs>(kColorDev.inv, tab);
  const size_t chunks = (size_t)(W + kRun - 1) / kRun;
  const size_t items = chunks * (size_t)H;
  const PicDst dst{nullptr, rgb, cb, cr};
  for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
    const size_t row = it / chunks;
    const int x0 = (int)(it % chunks) * kRun;
    const int n = W - x0 < kRun ? W - x0 : kRun;
    const size_t o = row * (size_t)W + x0;
    if (y_f32) {
      float v[1][kRun];
      load_floats(y_f32 + (long long)row * y_sh + (long long)x0 * y_sw, y_sw, n, v[0]);
      store_run<1, kDstYcc>(v, run_mask(n), n, o, 0, dst, tab);
    } else {
      const bool full = n == kRun;
      unsigned yw[4], bw[4], rw[4], w[12];
      load_bytes<4>(y_u8 + o, full && aligned16(y_u8 + o), n, yw);
      load_bytes<4>(cb + o, full && aligned16(cb + o), n, bw);
      load_bytes<4>(cr + o, full && aligned16(cr + o), n, rw);
#pragma unroll
      for (int q = 0; q < 12; ++q) w[q] = 0;
#pragma unroll
      for (int p = 0; p < kRun; ++p) {
        int r, g, b;
        ycc_to_rgb_px(tab, (int)get_byte(yw, p), (int)get_byte(bw, p), (int)get_byte(rw, p), r, g, b);
        put_rgb(w, p, r, g, b);
      }
      unsigned char* d = rgb + o * 3;
      store_bytes<12>(d, full && aligned16(d), n * 3, w);
    }
  }
}

// A dense image is one long row: every run of the flat pixel sequence then starts 16-byte aligned whatever the width
// (a 510-pixel RGB row is 1530 bytes: taken row by row, seven rows of eight would start unaligned), and only the last
// run of the image is a tail.
static void flatten_rows(bool dense, int& H, int& W) {
  if (!dense || (long long)H * W > 0x7fffffffLL) return;
  W *= H;
  H = 1;
}

static dim3 image_grid(int H, int W) { return run_grid((size_t)((W + kRun - 1) / kRun) * (size_t)H); }

}  // namespace srk

using namespace srk;

extern "C" int srk_rgb_to_ycc_host(const uint8_t* rgb, size_t n, uint8_t* ycc) {
  SRK_REQUIRE(rgb && ycc, "rgb_to_ycc_host: null pointer");
  for (size_t i = 0; i < n; ++i) {
    int y, cb, cr;
    rgb_to_ycc_px(kColorHost.fwd, rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], y, cb, cr);
    ycc[3 * i] = (uint8_t)y, ycc[3 * i + 1] = (uint8_t)cb, ycc[3 * i + 2] = (uint8_t)cr;
  }
  return SRK_OK;
}

extern "C" int srk_ycc_to_rgb_host(const uint8_t* ycc, size_t n, uint8_t* rgb) {
  SRK_REQUIRE(ycc && rgb, "ycc_to_rgb_host: null pointer");
  for (size_t i = 0; i < n; ++i) {
    int r, g, b;
    ycc_to_rgb_px(kColorHost.inv, ycc[3 * i], ycc[3 * i + 1], ycc[3 * i + 2], r, g, b);
    rgb[3 * i] = (uint8_t)r, rgb[3 * i + 1] = (uint8_t)g, rgb[3 * i + 2] = (uint8_t)b;
  }
  return SRK_OK;
}

extern "C" int srk_rgb_to_ycc_u8(const uint8_t* rgb, int64_t row_stride, int H, int W, float* y_f32, uint8_t* y_u8,
                                 uint8_t* cbcr, void* stream) {
  SRK_REQUIRE(rgb, "rgb_to_ycc_u8: null image pointer");
  SRK_REQUIRE(H > 0 && W > 0, "rgb_to_ycc_u8: non-positive dims (%d x %d)", H, W);
  SRK_REQUIRE(row_stride >= (int64_t)W * 3, "rgb_to_ycc_u8: row stride %lld < 3 * W = %lld", (long long)row_stride,
              (long long)W * 3);
  SRK_REQUIRE(y_f32 || y_u8 || cbcr, "rgb_to_ycc_u8: no output requested");
  flatten_rows(row_stride == (int64_t)W * 3, H, W);
  hipLaunchKernelGGL(k_rgb_to_ycc, image_grid(H, W), dim3(256), 0, (hipStream_t)stream, rgb, (long long)row_stride, H, W, y_f32,
                     y_u8, cbcr);
  return check_launch("rgb_to_ycc_u8");
}

extern "C" int srk_ycc_to_rgb_u8(const float* y_f32, int64_t y_row_stride, int64_t y_px_stride, const uint8_t* y_u8,
                                 const uint8_t* cb, const uint8_t* cr, uint8_t* rgb, int H, int W, void* stream) {
  SRK_REQUIRE((y_f32 != nullptr) != (y_u8 != nullptr), "ycc_to_rgb_u8: exactly one of y_f32 / y_u8 must be given");
  SRK_REQUIRE(cb && cr && rgb, "ycc_to_rgb_u8: null pointer");
  SRK_REQUIRE(H > 0 && W > 0, "ycc_to_rgb_u8: non-positive dims (%d x %d)", H, W);
  SRK_REQUIRE(!y_f32 || (y_row_stride >= 0 && y_px_stride >= 0), "ycc_to_rgb_u8: negative Y strides");
  flatten_rows(!y_f32 || y_row_stride == (int64_t)W * y_px_stride, H, W);
  hipLaunchKernelGGL(k_ycc_to_rgb, image_grid(H, W), dim3(256), 0, (hipStream_t)stream, y_f32, (long long)y_row_stride,
                     (long long)y_px_stride, y_u8, cb, cr, rgb, H, W);
  return check_launch("ycc_to_rgb_u8");
}

extern "C" int srk_float_to_u8_image(const float* x, int64_t c_stride, int64_t row_stride, int64_t px_stride, uint8_t* out,
                                     int C, int H, int W, void* stream) {
  SRK_REQUIRE(x && out, "float_to_u8_image: null pointer");
  SRK_REQUIRE(C == 1 || C == 3, "float_to_u8_image: C must be 1 or 3 (got %d)", C);
  SRK_REQUIRE(H > 0 && W > 0, "float_to_u8_image: non-positive dims (%d x %d)", H, W);
  SRK_REQUIRE(c_stride >= 0 && row_stride >= 0 && px_stride >= 0, "float_to_u8_image: negative strides");
  flatten_rows(row_stride == (int64_t)W * px_stride, H, W);
  launch_pic(C, kDstF32, [&](auto c, auto) {
    hipLaunchKernelGGL(k_to_u8<c()>, image_grid(H, W), dim3(256), 0, (hipStream_t)stream, x,
                       Strides4{0, c_stride, row_stride, px_stride}, out, H, W);
  });
  return check_launch("float_to_u8_image");
}
