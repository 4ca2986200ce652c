// What the video kernels (video.hip) and their host twins share: the planar 8-bit frame of a YUV4MPEG2 stream and the
// per-pixel arithmetic on it.  Everything here is __host__ __device__ and integer or fp32: the device kernels and
// srk_yuv_unpack_host / srk_yuv_pack_host compile the very same expressions (as jpeg_common.h and color_common.h do), so
// the CPU suite and a sanitizer run pin the arithmetic without a GPU.
//
// A frame is Y [H][W], then (4:2:0) Cb and Cr [ceil(H/2)][ceil(W/2)] or (4:4:4) Cb and Cr [H][W], or (mono) nothing,
// all dense and 8-bit; frames follow each other at a byte stride >= the frame's size and start at ANY address (a
// Y4M payload of a 6 x 4 stream is 36 bytes: frame 1 starts at byte 36).  Samples are full-range JFIF values, as the
// picture path takes them: the colour conversions are Pillow's tables (color_common.h).
#ifndef SRK_VIDEO_COMMON_H_
#define SRK_VIDEO_COMMON_H_
#include "color_common.h"

namespace srk {

struct YuvGeom {
  size_t ypix, cpix;   // samples of the Y plane and of ONE chroma plane (0: mono)
  int ch, cw;          // the chroma plane's size
  size_t bytes;        // ypix + 2 cpix
};

// sub: SRK_YUV_420 / SRK_YUV_444 / SRK_YUV_MONO
__host__ __device__ inline YuvGeom yuv_geom(int H, int W, int sub) {
  YuvGeom g;
  g.ypix = (size_t)H * (size_t)W;
  g.ch = sub == SRK_YUV_420 ? (H + 1) / 2 : (sub == SRK_YUV_444 ? H : 0);
  g.cw = sub == SRK_YUV_420 ? (W + 1) / 2 : (sub == SRK_YUV_444 ? W : 0);
  g.cpix = (size_t)g.ch * (size_t)g.cw;
  g.bytes = g.ypix + 2 * g.cpix;
  return g;
}

// ToTensor's division (k_rgb_to_ycc makes the same one)
__host__ __device__ __forceinline__ float yuv_to_unit(int v) { return (float)v / 255.0f; }

// one pixel of the RGB front: Pillow's YCbCr -> RGB (k_ycc_to_rgb's arithmetic), then ToTensor
__host__ __device__ __forceinline__ void yuv_unpack_px(const int16_t* inv, int y, int cb, int cr, float& r, float& g, float& b) {
  int ri, gi, bi;
  ycc_to_rgb_px(inv, y, cb, cr, ri, gi, bi);
  r = yuv_to_unit(ri), g = yuv_to_unit(gi), b = yuv_to_unit(bi);
}

// one pixel of the RGB tail: store_run's quantisation of the three channels, then Pillow's RGB -> YCbCr
__host__ __device__ __forceinline__ void yuv_pack_px(const int16_t* fwd, float r, float g, float b, int& y, int& cb, int& cr) {
  rgb_to_ycc_px(fwd, (int)quant_u8(r), (int)quant_u8(g), (int)quant_u8(b), y, cb, cr);
}

// Image.resize((W / 2, H / 2), Image.BOX) of an 8-bit plane, one output sample from its 2 x 2 quad (a b / c d).  Pillow
// resamples in two passes and rounds to 8 bits after each: along the row first, then down the column.  That is NOT the
// four-sample mean (a + b + c + d + 2) >> 2.
__host__ __device__ __forceinline__ int yuv_box_pair(int a, int b) { return (a + b + 1) >> 1; }
__host__ __device__ __forceinline__ int yuv_box_quad(int a, int b, int c, int d) {
  return yuv_box_pair(yuv_box_pair(a, b), yuv_box_pair(c, d));
}

}  // namespace srk
#endif  // SRK_VIDEO_COMMON_H_
