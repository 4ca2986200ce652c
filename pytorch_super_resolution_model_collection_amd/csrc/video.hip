// The front and the tail of test_video (sr_trainers.py): a batch of planar 8-bit frames of a YUV4MPEG2 stream -> the
// net's fp32 input, and the net's fp32 output -> a batch of planar 8-bit output frames, one launch each, so that a batch
// goes from file bytes to file bytes without a host pass.  The frame and the per-pixel arithmetic: video_common.h.
//
//   k_yuv_unpack<1>     Y model: Y / 255.0f (ToTensor's division, as k_rgb_to_ycc makes it) -> [N][1][H][W]; the chroma
//                       is not read.
//   k_yuv_unpack<3>     RGB model: Y of the frame + full-resolution Cb / Cr (4:4:4: the frame's own planes; 4:2:0: the
//                       planes srk_img_resize_u8 made of the frame's, bicubic; mono: the constant 128) through Pillow's
//                       YCbCr -> RGB tables (k_ycc_to_rgb's arithmetic), / 255.0f -> [N][3][H][W].
//   k_yuv_pack_y        Y model: store_run's quantisation of the net's Y' into the frames' Y planes, and the copy of the
//                       2 N resized chroma planes ([2][N][ch][cw], srk_img_resize_u8's dense output) into their slots.
//   k_yuv_pack_rgb      RGB model, 4:4:4 and mono: quantise R, G, B, Pillow's RGB -> YCbCr tables, write Y' (and Cb', Cr').
//   k_yuv_pack_rgb420   RGB model, 4:2:0: a thread owns a run of 16 chroma samples = 16 quads of 2 x 2 pixels; it writes
//                       their Y' and Pillow's resize((OW / 2, OH / 2), Image.BOX) of the full-resolution chroma, which
//                       never reaches memory (yuv_box_quad: rounded after each pass, not the four-sample mean).
//
// Streaming kernels after color.hip: a thread owns a run of 16 pixels; an access is 16 bytes wide where its pointer is
// 16-byte aligned and the run complete, scalar otherwise, decided per pointer -- a frame payload starts anywhere.  A
// plane is walked as ONE row of H * W pixels wherever the arithmetic has no use for the row (everything but the quads),
// so that an odd width does not misalign every other row.  Tables come from kColorDev through LDS; no scratch, no
// atomics, no floating-point colour coefficient on the device.  Net outputs are addressed through four element strides:
// a channels-last output is read in place.
#include "video_common.h"

namespace srk {

__device__ __forceinline__ void put_byte(unsigned* w, int k, int v) { w[k >> 2] |= (unsigned)v << ((k & 3) * 8); }

template <int C>
__global__ __launch_bounds__(256) void k_yuv_unpack(const unsigned char* __restrict__ frames, long long fstride, int N,
                                                    size_t pix, const unsigned char* __restrict__ cb0,
                                                    const unsigned char* __restrict__ cr0, long long cstride,
                                                    float* __restrict__ out) {
  __shared__ alignas(16) int16_t tab[C == 3 ? kInvTabs * 256 : 8];
  if (C == 3) stage_tables<kInvTabs>(kColorDev.inv, tab);
  const size_t chunks = (pix + kRun - 1) / kRun;
  const size_t items = chunks * (size_t)N;
  for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
    const long long n = (long long)(it / chunks);
    const size_t p0 = (it % chunks) * kRun;
    const int cnt = pix - p0 < (size_t)kRun ? (int)(pix - p0) : kRun;
    const bool full = cnt == kRun;
    const unsigned char* ys = frames + n * fstride + p0;
    unsigned yw[4];
    load_bytes<4>(ys, full && aligned16(ys), cnt, yw);
    float v[C][kRun];
    if (C == 1) {
#pragma unroll
      for (int p = 0; p < kRun; ++p) v[0][p] = yuv_to_unit((int)get_byte(yw, p));
    } else {
      unsigned bw[4] = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
      unsigned rw[4] = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
      if (cb0) {
        const unsigned char* bs = cb0 + n * cstride + p0;
        const unsigned char* rs = cr0 + n * cstride + p0;
        load_bytes<4>(bs, full && aligned16(bs), cnt, bw);
        load_bytes<4>(rs, full && aligned16(rs), cnt, rw);
      }
#pragma unroll
      for (int p = 0; p < kRun; ++p)
        yuv_unpack_px(tab, (int)get_byte(yw, p), (int)get_byte(bw, p), (int)get_byte(rw, p), v[0][p], v[C > 1 ? 1 : 0][p],
                      v[C > 2 ? 2 : 0][p]);
    }
    const PicDst dst{out + (size_t)n * C * pix, nullptr, nullptr, nullptr};
    store_run<C, kDstF32>(v, run_mask(cnt), cnt, p0, pix, dst, nullptr);
  }
}

// y: [N][1][H][W] through s (the launcher hands a dense plane over as one row); chroma: [2][N][cpix] or cpix == 0
__global__ __launch_bounds__(256) void k_yuv_pack_y(const float* __restrict__ y, Strides4 s, int N, int H, int W,
                                                    const unsigned char* __restrict__ chroma, size_t cpix,
                                                    unsigned char* __restrict__ frames, long long fstride) {
  const size_t ychunks = ((size_t)W + kRun - 1) / kRun;
  const size_t yitems = ychunks * (size_t)H;
  const size_t cchunks = (cpix + kRun - 1) / kRun;
  const size_t per = yitems + 2 * cchunks;
  const size_t items = per * (size_t)N;
  const size_t ypix = (size_t)H * W;
  for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
    const long long n = (long long)(it / per);
    size_t r = it % per;
    unsigned char* f = frames + n * fstride;
    unsigned w[4] = {0, 0, 0, 0};
    if (r < yitems) {
      const long long row = (long long)(r / ychunks);
      const int x0 = (int)(r % ychunks) * kRun;
      const int cnt = W - x0 < kRun ? W - x0 : kRun;
      float v[kRun];
      load_floats(y + n * s.n + row * s.h + (long long)x0 * s.w, s.w, cnt, v);
#pragma unroll
      for (int p = 0; p < kRun; ++p) put_byte(w, p, (int)quant_u8(v[p]));
      unsigned char* d = f + (size_t)row * W + x0;
      store_bytes<4>(d, cnt == kRun && aligned16(d), cnt, w);
    } else {
      r -= yitems;
      const size_t k = r / cchunks;
      const size_t p0 = (r % cchunks) * kRun;
      const int cnt = cpix - p0 < (size_t)kRun ? (int)(cpix - p0) : kRun;
      const unsigned char* src = chroma + (k * (size_t)N + (size_t)n) * cpix + p0;
      unsigned char* d = f + ypix + k * cpix + p0;
      load_bytes<4>(src, cnt == kRun && aligned16(src), cnt, w);
      store_bytes<4>(d, cnt == kRun && aligned16(d), cnt, w);
    }
  }
}

// x: [N][3][H][W] through s (a dense picture comes as one row); CHROMA: 4:4:4 (Cb', Cr' as they are), else mono (Y' only)
template <bool CHROMA>
__global__ __launch_bounds__(256) void k_yuv_pack_rgb(const float* __restrict__ x, Strides4 s, int N, int H, int W,
                                                      unsigned char* __restrict__ frames, long long fstride) {
  __shared__ alignas(16) int16_t tab[kFwdTabs * 256];
  stage_tables<kFwdTabs>(kColorDev.fwd, tab);
  const size_t chunks = ((size_t)W + kRun - 1) / kRun;
  const size_t per = chunks * (size_t)H;
  const size_t items = per * (size_t)N;
  const size_t ypix = (size_t)H * W;
  for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
    const long long n = (long long)(it / per);
    const size_t r = it % per;
    const long long row = (long long)(r / chunks);
    const int x0 = (int)(r % chunks) * kRun;
    const int cnt = W - x0 < kRun ? W - x0 : kRun;
    const bool full = cnt == kRun;
    float v[3][kRun];
    load_run<3>(x + n * s.n + row * s.h + (long long)x0 * s.w, s.c, s.w, cnt, v);
    unsigned yw[4] = {0, 0, 0, 0}, bw[4] = {0, 0, 0, 0}, rw[4] = {0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < kRun; ++p) {
      int yy, cb, cr;
      yuv_pack_px(tab, v[0][p], v[1][p], v[2][p], yy, cb, cr);
      put_byte(yw, p, yy), put_byte(bw, p, cb), put_byte(rw, p, cr);
    }
    unsigned char* d = frames + n * fstride + (size_t)row * W + x0;
    store_bytes<4>(d, full && aligned16(d), cnt, yw);
    if (CHROMA) {
      store_bytes<4>(d + ypix, full && aligned16(d + ypix), cnt, bw);
      store_bytes<4>(d + 2 * ypix, full && aligned16(d + 2 * ypix), cnt, rw);
    }
  }
}

// x: [N][3][H][W] through s, H and W even.  An item is a run of 16 chroma samples of one chroma row: 2 rows x 32 pixels,
// walked as two halves of 2 x 16.  Both loops are fully unrolled (the byte positions must be constants), and the compiler
// hoists the loads of all four 48-float runs ahead of the arithmetic: 234 VGPRs, two waves a SIMD, no scratch.
__global__ __launch_bounds__(256) void k_yuv_pack_rgb420(const float* __restrict__ x, Strides4 s, int N, int H, int W,
                                                         unsigned char* __restrict__ frames, long long fstride) {
  __shared__ alignas(16) int16_t tab[kFwdTabs * 256];
  stage_tables<kFwdTabs>(kColorDev.fwd, tab);
  const int CH = H / 2, CW = W / 2;
  const size_t cchunks = ((size_t)CW + kRun - 1) / kRun;
  const size_t per = cchunks * (size_t)CH;
  const size_t items = per * (size_t)N;
  const size_t ypix = (size_t)H * W, cpix = (size_t)CH * CW;
  for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
    const long long n = (long long)(it / per);
    const size_t r = it % per;
    const long long crow = (long long)(r / cchunks);
    const int cx0 = (int)(r % cchunks) * kRun;
    const int nc = CW - cx0 < kRun ? CW - cx0 : kRun;
    unsigned char* f = frames + n * fstride;
    unsigned bo[4] = {0, 0, 0, 0}, ro[4] = {0, 0, 0, 0};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int x0 = 2 * cx0 + kRun * half;
      const int cnt = W - x0 < kRun ? W - x0 : kRun;   // even, as W is
      if (cnt <= 0) continue;
      int hb[kRun / 2], hr[kRun / 2];   // the row pass of the upper row
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const long long row = 2 * crow + rr;
        float v[3][kRun];
        load_run<3>(x + n * s.n + row * s.h + (long long)x0 * s.w, s.c, s.w, cnt, v);
        unsigned yw[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < kRun / 2; ++j) {
          int y0, b0, r0, y1, b1, r1;
          yuv_pack_px(tab, v[0][2 * j], v[1][2 * j], v[2][2 * j], y0, b0, r0);
          yuv_pack_px(tab, v[0][2 * j + 1], v[1][2 * j + 1], v[2][2 * j + 1], y1, b1, r1);
          put_byte(yw, 2 * j, y0), put_byte(yw, 2 * j + 1, y1);
          const int b = yuv_box_pair(b0, b1), c = yuv_box_pair(r0, r1);
          if (rr == 0) {
            hb[j] = b, hr[j] = c;
          } else {
            put_byte(bo, (kRun / 2) * half + j, yuv_box_pair(hb[j], b));
            put_byte(ro, (kRun / 2) * half + j, yuv_box_pair(hr[j], c));
          }
        }
        unsigned char* d = f + (size_t)row * W + x0;
        store_bytes<4>(d, cnt == kRun && aligned16(d), cnt, yw);
      }
    }
    unsigned char* db = f + ypix + (size_t)crow * CW + cx0;
    store_bytes<4>(db, nc == kRun && aligned16(db), nc, bo);
    store_bytes<4>(db + cpix, nc == kRun && aligned16(db + cpix), nc, ro);
  }
}

// ---- what the device entry points and the host twins check alike ----

static int yuv_frames_ok(const char* what, int N, int H, int W, int sub, int C, int64_t frame_stride) {
  SRK_REQUIRE(N > 0 && H > 0 && W > 0, "%s: non-positive sizes (N = %d, %d x %d)", what, N, H, W);
  SRK_REQUIRE(sub == SRK_YUV_420 || sub == SRK_YUV_444 || sub == SRK_YUV_MONO, "%s: unknown subsampling code %d", what, sub);
  SRK_REQUIRE(C == 1 || C == 3, "%s: C must be 1 or 3 (got %d)", what, C);
  SRK_REQUIRE(sub != SRK_YUV_420 || (H % 2 == 0 && W % 2 == 0), "%s: a 4:2:0 frame of odd size (%d x %d) is refused", what, W, H);
  SRK_REQUIRE((long long)H * W <= 0x7fffffffLL, "%s: a frame of %d x %d is too large", what, W, H);
  const YuvGeom g = yuv_geom(H, W, sub);
  SRK_REQUIRE(frame_stride >= (int64_t)g.bytes, "%s: frame stride %lld < the frame's %lld bytes", what, (long long)frame_stride,
              (long long)g.bytes);
  return SRK_OK;
}

static int yuv_unpack_ok(const char* what, const void* frames, int64_t frame_stride, int N, int H, int W, int sub, int C,
                         const void* chroma_full, const void* out) {
  SRK_REQUIRE(frames && out, "%s: null pointer", what);
  if (int rc = yuv_frames_ok(what, N, H, W, sub, C, frame_stride)) return rc;
  SRK_REQUIRE(!(C == 3 && sub == SRK_YUV_420) || chroma_full, "%s: an RGB model on a 4:2:0 stream needs the full-resolution chroma planes",
              what);
  return SRK_OK;
}

static int yuv_pack_ok(const char* what, const void* x, const int64_t* strides, int N, int C, int OH, int OW, int sub,
                       const void* chroma, const void* frames, int64_t frame_stride) {
  SRK_REQUIRE(x && strides && frames, "%s: null pointer", what);
  if (int rc = yuv_frames_ok(what, N, OH, OW, sub, C, frame_stride)) return rc;
  SRK_REQUIRE(strides[0] >= 0 && strides[1] >= 0 && strides[2] >= 0 && strides[3] >= 0, "%s: negative strides", what);
  SRK_REQUIRE(!(C == 1 && sub != SRK_YUV_MONO) || chroma, "%s: a Y model on a colour stream needs the resized chroma planes", what);
  return SRK_OK;
}

static void flatten_plane(const Strides4& s, int& H, int& W) {
  if (s.h != (int64_t)W * s.w) return;
  W *= H;
  H = 1;
}

}  // namespace srk

using namespace srk;

extern "C" int srk_yuv_unpack(const uint8_t* frames, int64_t frame_stride, int N, int H, int W, int sub, int C,
                              const uint8_t* chroma_full, float* out, void* stream) {
  if (int rc = yuv_unpack_ok("yuv_unpack", frames, frame_stride, N, H, W, sub, C, chroma_full, out)) return rc;
  const YuvGeom g = yuv_geom(H, W, sub);
  const dim3 grid = run_grid((g.ypix + kRun - 1) / kRun * (size_t)N);
  if (C == 1) {
    hipLaunchKernelGGL(k_yuv_unpack<1>, grid, dim3(256), 0, (hipStream_t)stream, frames, (long long)frame_stride, N, g.ypix,
                       (const unsigned char*)nullptr, (const unsigned char*)nullptr, 0LL, out);
  } else {
    const unsigned char *cb = nullptr, *cr = nullptr;
    long long cstride = 0;
    if (sub == SRK_YUV_444) cb = frames + g.ypix, cr = frames + 2 * g.ypix, cstride = frame_stride;
    if (sub == SRK_YUV_420) cb = chroma_full, cr = chroma_full + (size_t)N * g.ypix, cstride = (long long)g.ypix;
    hipLaunchKernelGGL(k_yuv_unpack<3>, grid, dim3(256), 0, (hipStream_t)stream, frames, (long long)frame_stride, N, g.ypix, cb,
                       cr, cstride, out);
  }
  return check_launch("yuv_unpack");
}

extern "C" int srk_yuv_pack(const float* x, const int64_t* strides, int N, int C, int OH, int OW, int sub,
                            const uint8_t* chroma, uint8_t* frames, int64_t frame_stride, void* stream) {
  if (int rc = yuv_pack_ok("yuv_pack", x, strides, N, C, OH, OW, sub, chroma, frames, frame_stride)) return rc;
  const YuvGeom g = yuv_geom(OH, OW, sub);
  const Strides4 s = strides4(strides);
  int H = OH, W = OW;
  if (C == 1) {
    flatten_plane(s, H, W);
    const size_t per = (((size_t)W + kRun - 1) / kRun) * (size_t)H + 2 * ((g.cpix + kRun - 1) / kRun);
    hipLaunchKernelGGL(k_yuv_pack_y, run_grid(per * (size_t)N), dim3(256), 0, (hipStream_t)stream, x, s, N, H, W, chroma, g.cpix,
                       frames, (long long)frame_stride);
  } else if (sub == SRK_YUV_420) {
    const size_t per = (((size_t)g.cw + kRun - 1) / kRun) * (size_t)g.ch;
    hipLaunchKernelGGL(k_yuv_pack_rgb420, run_grid(per * (size_t)N), dim3(256), 0, (hipStream_t)stream, x, s, N, H, W, frames,
                       (long long)frame_stride);
  } else {
    flatten_plane(s, H, W);
    const dim3 grid = run_grid((((size_t)W + kRun - 1) / kRun) * (size_t)H * (size_t)N);
    if (sub == SRK_YUV_444)
      hipLaunchKernelGGL(k_yuv_pack_rgb<true>, grid, dim3(256), 0, (hipStream_t)stream, x, s, N, H, W, frames,
                         (long long)frame_stride);
    else
      hipLaunchKernelGGL(k_yuv_pack_rgb<false>, grid, dim3(256), 0, (hipStream_t)stream, x, s, N, H, W, frames,
                         (long long)frame_stride);
  }
  return check_launch("yuv_pack");
}

// The same two definitions on HOST pointers, pixel by pixel through video_common.h.

extern "C" int srk_yuv_unpack_host(const uint8_t* frames, int64_t frame_stride, int N, int H, int W, int sub, int C,
                                   const uint8_t* chroma_full, float* out) {
  if (int rc = yuv_unpack_ok("yuv_unpack_host", frames, frame_stride, N, H, W, sub, C, chroma_full, out)) return rc;
  const YuvGeom g = yuv_geom(H, W, sub);
  for (int n = 0; n < N; ++n) {
    const uint8_t* f = frames + (int64_t)n * frame_stride;
    float* o = out + (size_t)n * C * g.ypix;
    for (size_t p = 0; p < g.ypix; ++p) {
      if (C == 1) {
        o[p] = yuv_to_unit(f[p]);
        continue;
      }
      int cb = 128, cr = 128;
      if (sub == SRK_YUV_444) cb = f[g.ypix + p], cr = f[2 * g.ypix + p];
      if (sub == SRK_YUV_420) cb = chroma_full[(size_t)n * g.ypix + p], cr = chroma_full[((size_t)N + n) * g.ypix + p];
      yuv_unpack_px(kColorHost.inv, f[p], cb, cr, o[p], o[g.ypix + p], o[2 * g.ypix + p]);
    }
  }
  return SRK_OK;
}

extern "C" int srk_yuv_pack_host(const float* x, const int64_t* strides, int N, int C, int OH, int OW, int sub,
                                 const uint8_t* chroma, uint8_t* frames, int64_t frame_stride) {
  if (int rc = yuv_pack_ok("yuv_pack_host", x, strides, N, C, OH, OW, sub, chroma, frames, frame_stride)) return rc;
  const YuvGeom g = yuv_geom(OH, OW, sub);
  const Strides4 s = strides4(strides);
  for (int n = 0; n < N; ++n) {
    uint8_t* f = frames + (int64_t)n * frame_stride;
    const float* xn = x + (int64_t)n * s.n;
    auto px = [&](int row, int col, int& y, int& cb, int& cr) {
      const float* p = xn + (int64_t)row * s.h + (int64_t)col * s.w;
      yuv_pack_px(kColorHost.fwd, p[0], p[s.c], p[2 * s.c], y, cb, cr);
    };
    if (C == 1) {
      for (int row = 0; row < OH; ++row)
        for (int col = 0; col < OW; ++col) f[(size_t)row * OW + col] = (uint8_t)quant_u8(xn[(int64_t)row * s.h + (int64_t)col * s.w]);
      for (int k = 0; k < 2; ++k)
        for (size_t p = 0; p < g.cpix; ++p) f[g.ypix + k * g.cpix + p] = chroma[((size_t)k * N + n) * g.cpix + p];
    } else if (sub == SRK_YUV_420) {
      for (int crow = 0; crow < g.ch; ++crow)
        for (int cc = 0; cc < g.cw; ++cc) {
          int y[4], b[4], r[4];
          for (int q = 0; q < 4; ++q) {
            px(2 * crow + (q >> 1), 2 * cc + (q & 1), y[q], b[q], r[q]);
            f[(size_t)(2 * crow + (q >> 1)) * OW + 2 * cc + (q & 1)] = (uint8_t)y[q];
          }
          f[g.ypix + (size_t)crow * g.cw + cc] = (uint8_t)yuv_box_quad(b[0], b[1], b[2], b[3]);
          f[g.ypix + g.cpix + (size_t)crow * g.cw + cc] = (uint8_t)yuv_box_quad(r[0], r[1], r[2], r[3]);
        }
    } else {
      for (int row = 0; row < OH; ++row)
        for (int col = 0; col < OW; ++col) {
          int y, cb, cr;
          px(row, col, y, cb, cr);
          const size_t o = (size_t)row * OW + col;
          f[o] = (uint8_t)y;
          if (sub == SRK_YUV_444) f[g.ypix + o] = (uint8_t)cb, f[2 * g.ypix + o] = (uint8_t)cr;
        }
    }
  }
  return SRK_OK;
}
