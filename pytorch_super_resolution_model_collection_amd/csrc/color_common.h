// What the kernels of the picture tail share (color.hip: colour conversion and quantisation; tile.hip: the stitch of
// tiled results; dihedral.hip: the merge of the self-ensemble -- both quantise and convert on the way): Pillow's colour
// tables, the quantisation expression of ToPILImage, the destination of a picture (PicDst), and for the byte-stream
// kernels the 16-pixel run: its accessors, its reader (load_run) and its writer (store_run).  See color.hip for the
// derivation of the tables and the access pattern.
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

// copies NT consecutive 256-entry int16 tables from constant memory into LDS (blockDim.x == THREADS)
template <int NT, int THREADS = 256>
__device__ __forceinline__ void stage_tables(const int16_t* __restrict__ src, int16_t* dst) {
  const unsigned* s = reinterpret_cast<const unsigned*>(src);
  unsigned* d = reinterpret_cast<unsigned*>(dst);
  for (int i = threadIdx.x; i < NT * 128; i += THREADS) d[i] = s[i];
  __syncthreads();
}

// Where a picture goes.  The kernels that end the tail (k_tile_stitch, k_dihedral_merge) are instantiated per kind and
// take the pointers of all kinds in one PicDst; a launch fills those of its kind.
enum { kDstF32 = 0,    // fp32 planar [C][H][W]: f32
       kDstU8 = 1,     // interleaved 8-bit [H][W][C], quantised with quant_u8: u8
       kDstYcc = 2 };  // C = 1: Y quantised, + 8-bit Cb / Cr planes [H][W] (cb, cr) -> interleaved 8-bit RGB: u8
struct PicDst {
  float* f32;
  unsigned char* u8;
  const unsigned char* cb;
  const unsigned char* cr;
};

// bytes 3 k .. 3 k + 2 of the words w[] = pixel k of an interleaved RGB run
__device__ __forceinline__ void put_rgb(unsigned* w, int k, int r, int g, int b) {
  w[(3 * k) >> 2] |= (unsigned)r << (((3 * k) & 3) * 8);
  w[(3 * k + 1) >> 2] |= (unsigned)g << (((3 * k + 1) & 3) * 8);
  w[(3 * k + 2) >> 2] |= (unsigned)b << (((3 * k + 2) & 3) * 8);
}

// `own` of a run whose first n pixels exist
__device__ __forceinline__ unsigned run_mask(int n) { return n == kRun ? 0xffffu : (1u << n) - 1u; }

// A run of n pixels of one row of a [C][H][W] picture (element strides sc, sw) starting at s -> v[c][k], channel by channel
template <int C>
__device__ __forceinline__ void load_planes(const float* __restrict__ s, long long sc, long long sw, int n, float (&v)[C][kRun]) {
#pragma unroll
  for (int c = 0; c < C; ++c) load_floats(s + c * sc, sw, n, v[c]);
}
// ... taking a complete run of a channels-last RGB picture as what it is in memory, 48 consecutive floats
template <int C>
__device__ __forceinline__ void load_run(const float* __restrict__ s, long long sc, long long sw, int n, float (&v)[C][kRun]) {
  if (C == 3 && sc == 1 && sw == 3 && n == kRun && aligned16(s)) {
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      const float4 f = reinterpret_cast<const float4*>(s)[q];
      const int e = 4 * q;   // element e of the run's 48 floats is pixel e / C, channel e % C
      v[e % C][e / C] = f.x, v[(e + 1) % C][(e + 1) / C] = f.y, v[(e + 2) % C][(e + 2) / C] = f.z,
                   v[(e + 3) % C][(e + 3) / C] = f.w;
    }
  } else {
    load_planes<C>(s, sc, sw, n, v);
  }
}

// The run v[c][k] to pixels p0 .. p0 + nrun of a dense picture of `plane` pixels; bit k of `own` says that pixel k is
// written.  fp32: planar stores.  8-bit: quantised and interleaved, or (kDstYcc; ctab = ColorTables::inv) converted with
// the run's chroma.  16-byte stores when all 16 pixels are owned and the pointer is aligned, else pixel by pixel.
template <int C, int DST>
__device__ __forceinline__ void store_run(const float (&v)[C][kRun], unsigned own, int nrun, size_t p0, size_t plane,
                                          const PicDst& dst, const int16_t* ctab) {
  constexpr int OC = DST == kDstYcc ? 3 : C;   // channels of the 8-bit destination
  const bool all = own == 0xffffu;
  if (DST == kDstF32) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float* d = dst.f32 + c * plane + p0;
      if (all && aligned16(d)) {
#pragma unroll
        for (int q = 0; q < kRun / 4; ++q)
          reinterpret_cast<float4*>(d)[q] = make_float4(v[c][4 * q], v[c][4 * q + 1], v[c][4 * q + 2], v[c][4 * q + 3]);
      } else {
#pragma unroll
        for (int k = 0; k < kRun; ++k)
          if (own >> k & 1u) d[k] = v[c][k];
      }
    }
  } else {
    unsigned w[4 * OC];
#pragma unroll
    for (int q = 0; q < 4 * OC; ++q) w[q] = 0;
    if (DST == kDstU8) {
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
          const int b = k * C + c;
          w[b >> 2] |= quant_u8(v[c][k]) << ((b & 3) * 8);
        }
    } else {
      unsigned bw[4], rw[4];
      load_bytes<4>(dst.cb + p0, nrun == kRun && aligned16(dst.cb + p0), nrun, bw);
      load_bytes<4>(dst.cr + p0, nrun == kRun && aligned16(dst.cr + p0), nrun, rw);
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        int r, g, b;
        ycc_to_rgb_px(ctab, (int)quant_u8(v[0][k]), (int)get_byte(bw, k), (int)get_byte(rw, k), r, g, b);
        put_rgb(w, k, r, g, b);
      }
    }
    unsigned char* d = dst.u8 + p0 * OC;
    if (all) {
      store_bytes<4 * OC>(d, aligned16(d), kRun * OC, w);
    } else {
#pragma unroll
      for (int k = 0; k < kRun; ++k)
        if (own >> k & 1u) {
#pragma unroll
          for (int c = 0; c < OC; ++c) d[k * OC + c] = (unsigned char)get_byte(w, k * OC + c);
        }
    }
  }
}

// ---- host side of the launchers ----

// one thread per run, 256 a block, grid-stride beyond 65535 blocks
inline dim3 run_grid(size_t runs) {
  const size_t nb = (runs + 255) / 256;
  return dim3((unsigned)(nb > 65535 ? 65535 : (nb < 1 ? 1 : nb)));
}

// f(integral_constant C, integral_constant DST) for the instantiation that (C in {1, 3}, dst) names; a launcher whose
// kernel has no destination passes kDstF32 and ignores the second argument.  (3, kDstYcc) does not exist: pic_dst_ok.
template <typename F>
inline void launch_pic(int C, int dst, F&& f) {
  typedef std::integral_constant<int, 1> c1;
  typedef std::integral_constant<int, 3> c3;
  if (dst == kDstYcc)
    f(c1{}, std::integral_constant<int, kDstYcc>{});
  else if (dst == kDstU8)
    C == 3 ? f(c3{}, std::integral_constant<int, kDstU8>{}) : f(c1{}, std::integral_constant<int, kDstU8>{});
  else
    C == 3 ? f(c3{}, std::integral_constant<int, kDstF32>{}) : f(c1{}, std::integral_constant<int, kDstF32>{});
}

// the chroma planes of an 8-bit destination
inline int pic_dst_ok(const char* what, int C, const void* cb, const void* cr) {
  SRK_REQUIRE((cb != nullptr) == (cr != nullptr), "%s: cb and cr come together", what);
  SRK_REQUIRE(!cb || C == 1, "%s: chroma planes go with a Y output (C = 1), got C = %d", what, C);
  return SRK_OK;
}

}  // namespace srk
#endif  // SRK_COLOR_COMMON_H_
