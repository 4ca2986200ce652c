// What the byte-stream kernels of the picture tail share (color.hip: colour conversion and quantisation; tile.hip: the
// stitch of tiled results, which quantises and converts on the way): Pillow's colour tables, the quantisation expression
// of ToPILImage, and the 16-pixel-run accessors.  See color.hip for the derivation of the tables and the access pattern.
#ifndef SRK_COLOR_COMMON_H_
#define SRK_COLOR_COMMON_H_
#include "srk_common.h"

namespace srk {

// 256-entry int16 tables, contiguous per direction.
//   fwd (RGB -> YCbCr), unshifted 6-bit fixed-point terms: y_r, y_g, y_b, cb_r, cb_g, cr_g, cr_b
//   inv (YCbCr -> RGB): r_cr and b_cb already shifted (one term each), then g_cb and g_cr unshifted (summed before the shift)
constexpr int kFwdTabs = 7, kInvTabs = 4;
struct alignas(16) ColorTables {
  int16_t fwd[kFwdTabs * 256];
  int16_t inv[kInvTabs * 256];
};

constexpr int color_T(double c, int i) { return (int)(c * 64 * i + 0.5); }

constexpr ColorTables make_color_tables() {
  ColorTables t{};
  for (int i = 0; i < 256; ++i) {
    t.fwd[i] = (int16_t)color_T(.299, i);
    t.fwd[256 + i] = (int16_t)color_T(.587, i);
    t.fwd[512 + i] = (int16_t)color_T(.114, i);
    t.fwd[768 + i] = (int16_t)color_T(-.16874, i);
    t.fwd[1024 + i] = (int16_t)color_T(-.33126, i);
    t.fwd[1280 + i] = (int16_t)color_T(-.41869, i);
    t.fwd[1536 + i] = (int16_t)color_T(-.08131, i);
    t.inv[i] = (int16_t)(color_T(1.402, i - 128) >> 6);
    t.inv[256 + i] = (int16_t)(color_T(1.772, i - 128) >> 6);
    t.inv[512 + i] = (int16_t)color_T(-.34414, i - 128);
    t.inv[768 + i] = (int16_t)color_T(-.71414, i - 128);
  }
  return t;
}

static constexpr ColorTables kColorHost = make_color_tables();
__constant__ const ColorTables kColorDev = make_color_tables();

__host__ __device__ __forceinline__ int color_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// `fwd`: ColorTables::fwd (host: kColorHost.fwd; device: the LDS copy)
__host__ __device__ __forceinline__ void rgb_to_ycc_px(const int16_t* fwd, int r, int g, int b, int& y, int& cb, int& cr) {
  y = (fwd[r] + fwd[256 + g] + fwd[512 + b]) >> 6;
  cb = ((fwd[768 + r] + fwd[1024 + g] + 32 * b) >> 6) + 128;
  cr = ((32 * r + fwd[1280 + g] + fwd[1536 + b]) >> 6) + 128;
}
// `inv`: ColorTables::inv
__host__ __device__ __forceinline__ void ycc_to_rgb_px(const int16_t* inv, int y, int cb, int cr, int& r, int& g, int& b) {
  r = color_clip8(y + inv[cr]);
  g = color_clip8(y + ((inv[512 + cb] + inv[768 + cr]) >> 6));
  b = color_clip8(y + inv[256 + cb]);
}

// ToPILImage after clamp(0, 1) (edsr.py:305-306): pic.mul(255).byte() -- fp32 product, truncation; NaN -> 0 (fmaxf
// returns its non-NaN operand).  Host too: srk_ssim_host quantises with the very expression.
__host__ __device__ __forceinline__ unsigned quant_u8(float v) {
  return (unsigned)(fminf(fmaxf(v, 0.f), 1.f) * 255.0f);
}

constexpr int kRun = 16;  // pixels per thread

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__device__ __forceinline__ unsigned get_byte(const unsigned* w, int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 255u; }

// n_words x 4 bytes from p into w[]: 16-byte loads when `wide`, else `nbytes` scalar loads (the rest of w[] is zero)
template <int NW>
__device__ __forceinline__ void load_bytes(const unsigned char* __restrict__ p, bool wide, int nbytes, unsigned (&w)[NW]) {
  if (wide) {
#pragma unroll
    for (int q = 0; q < NW / 4; ++q) {
      const uint4 v = reinterpret_cast<const uint4*>(p)[q];
      w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < NW; ++q) w[q] = 0;
#pragma unroll
    for (int k = 0; k < NW * 4; ++k)
      if (k < nbytes) w[k >> 2] |= (unsigned)p[k] << ((k & 3) * 8);
  }
}
template <int NW>
__device__ __forceinline__ void store_bytes(unsigned char* __restrict__ p, bool wide, int nbytes, const unsigned (&w)[NW]) {
  if (wide) {
#pragma unroll
    for (int q = 0; q < NW / 4; ++q)
      reinterpret_cast<uint4*>(p)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < NW * 4; ++k)
      if (k < nbytes) p[k] = (unsigned char)get_byte(w, k);
  }
}
// a run of fp32 values addressed through an element stride: 16-byte loads when dense and aligned
__device__ __forceinline__ void load_floats(const float* __restrict__ p, long long stride, int n, float (&v)[kRun]) {
  if (n == kRun && stride == 1 && aligned16(p)) {
#pragma unroll
    for (int q = 0; q < kRun / 4; ++q) {
      const float4 f = reinterpret_cast<const float4*>(p)[q];
      v[4 * q] = f.x, v[4 * q + 1] = f.y, v[4 * q + 2] = f.z, v[4 * q + 3] = f.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kRun; ++k) v[k] = k < n ? p[k * stride] : 0.f;
  }
}

// copies NT consecutive 256-entry int16 tables from constant memory into LDS (blockDim.x == 256)
template <int NT>
__device__ __forceinline__ void stage_tables(const int16_t* __restrict__ src, int16_t* dst) {
  const unsigned* s = reinterpret_cast<const unsigned*>(src);
  unsigned* d = reinterpret_cast<unsigned*>(dst);
  for (int i = threadIdx.x; i < NT * 128; i += 256) d[i] = s[i];
  __syncthreads();
}

}  // namespace srk
#endif  // SRK_COLOR_COMMON_H_
