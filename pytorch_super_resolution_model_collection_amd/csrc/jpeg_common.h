// The JPEG round trip y = decode(encode(x, Q)) of one 8-bit picture as the kernel (jpeg.hip: k_jpeg_u8) and its host twin
// (srk_jpeg_u8_host) share it: libjpeg's baseline path without the lossless entropy coder, int32 end to end.  One body per
// step, compiled for both sides; the two differ only in who walks the 8 x 8 blocks.  include/srk.h, DESIGN.md 24.
#ifndef SRK_JPEG_COMMON_H_
#define SRK_JPEG_COMMON_H_
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace srk {

__host__ __device__ __forceinline__ int jpeg_min(int a, int b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ int jpeg_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__host__ __device__ __forceinline__ int jpeg_descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

// Entry k (natural order) of the Annex-K table (chroma 0: luminance) scaled to quality Q, Q clamped to 1..100.
__host__ __device__ __forceinline__ int jpeg_quant(int Q, int chroma, int k) {
  static constexpr uint8_t kBase[2][64] = {
      {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
       14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
      {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
       47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
       99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
  Q = jpeg_clamp(Q, 1, 100);
  const int s = Q < 50 ? 5000 / Q : 200 - 2 * Q;
  return jpeg_clamp(((int)kBase[chroma][k] * s + 50) / 100, 1, 255);
}

// One picture of the call: C dense planes [H][W]; sub 1 = 4:2:0, color 1 = the planes are R, G, B.
struct JpegPic {
  const uint8_t* x;
  int C, H, W, sub, color;
};

// Component comp (0 Y, 1 Cb, 2 Cr) of the pixel (y, x), both inside the picture.
__host__ __device__ __forceinline__ int jpeg_full(const JpegPic& p, int comp, int y, int x) {
  const size_t o = (size_t)y * p.W + x, plane = (size_t)p.H * p.W;
  if (!p.color) return p.x[comp * plane + o];
  const int r = p.x[o], g = p.x[plane + o], b = p.x[2 * plane + o];
  if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// Sample (i, j) of component comp's padded plane, i, j >= 0 in that plane's own (for 4:2:0 chroma: shrunk) coordinates.
// Full-size planes replicate their last row and column.  The chroma shrink replicates the source's last column, gives an
// odd height its last row once more, and then replicates the SHRUNK plane's last row: i is clamped in shrunk rows.
__host__ __device__ __forceinline__ int jpeg_sample(const JpegPic& p, int comp, int i, int j) {
  if (comp == 0 || !p.sub) return jpeg_full(p, comp, jpeg_min(i, p.H - 1), jpeg_min(j, p.W - 1));
  i = jpeg_min(i, ((p.H + 1) >> 1) - 1);
  const int y0 = 2 * i, y1 = jpeg_min(2 * i + 1, p.H - 1), x0 = jpeg_min(2 * j, p.W - 1), x1 = jpeg_min(2 * j + 1, p.W - 1);
  return (jpeg_full(p, comp, y0, x0) + jpeg_full(p, comp, y0, x1) + jpeg_full(p, comp, y1, x0) + jpeg_full(p, comp, y1, x1) +
          1 + (j & 1)) >> 2;
}

// jfdctint's butterfly on eight values in place.  first: the row pass (outputs scaled up by 2 bits); else the column pass.
__host__ __device__ __forceinline__ void jpeg_fdct8(int d[8], bool first) {
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int n = first ? 11 : 15;
  d[0] = first ? (t10 + t11) * 4 : jpeg_descale(t10 + t11, 2);      // (* 4, * 8192: the shifts << 2, << 13 of libjpeg,
  d[4] = first ? (t10 - t11) * 4 : jpeg_descale(t10 - t11, 2);      //  written so that a negative value is no left shift)
  const int e = (t12 + t13) * 4433;
  d[2] = jpeg_descale(e + t13 * 6270, n);
  d[6] = jpeg_descale(e - t12 * 15137, n);
  const int z5 = (t4 + t6 + t5 + t7) * 9633;
  const int z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995, z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
  d[7] = jpeg_descale(t4 * 2446 + z1 + z3, n);
  d[5] = jpeg_descale(t5 * 16819 + z2 + z4, n);
  d[3] = jpeg_descale(t6 * 25172 + z2 + z3, n);
  d[1] = jpeg_descale(t7 * 12299 + z1 + z4, n);
}

// jidctint's butterfly on eight coefficients in place, results descaled by n bits (11: column pass, 18: row pass).
__host__ __device__ __forceinline__ void jpeg_idct8(int c[8], int n) {
  const int e = (c[2] + c[6]) * 4433;
  const int e2 = e - c[6] * 15137, e3 = e + c[2] * 6270;
  const int e0 = (c[0] + c[4]) * 8192, e1 = (c[0] - c[4]) * 8192;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  const int a0 = c[7], a1 = c[5], a2 = c[3], a3 = c[1];
  const int z5 = (a0 + a2 + a1 + a3) * 9633;
  const int z1 = (a0 + a3) * -7373, z2 = (a1 + a2) * -20995, z3 = (a0 + a2) * -16069 + z5, z4 = (a1 + a3) * -3196 + z5;
  const int o0 = a0 * 2446 + z1 + z3, o1 = a1 * 16819 + z2 + z4, o2 = a2 * 25172 + z2 + z3, o3 = a3 * 12299 + z1 + z4;
  c[0] = jpeg_descale(t10 + o3, n);
  c[7] = jpeg_descale(t10 - o3, n);
  c[1] = jpeg_descale(t11 + o2, n);
  c[6] = jpeg_descale(t11 - o2, n);
  c[2] = jpeg_descale(t12 + o1, n);
  c[5] = jpeg_descale(t12 - o1, n);
  c[3] = jpeg_descale(t13 + o0, n);
  c[4] = jpeg_descale(t13 - o0, n);
}

// Quantise the DCT coefficient c (scaled by 8) under table entry t and dequantise it again.
__host__ __device__ __forceinline__ int jpeg_requant(int c, int t) {
  const int d = t << 3, q = ((c < 0 ? -c : c) + (d >> 1)) / d;
  return (c < 0 ? -q : q) * t;
}

// The middle of a block between the two transposes, on column r of it: forward column pass, quantisation under the column
// r of the table qt[64], inverse column pass (jidctint takes columns first, so no transpose lies between them).
__host__ __device__ __forceinline__ void jpeg_block_column(int v[8], const int* qt, int r) {
  jpeg_fdct8(v, false);
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = jpeg_requant(v[k], qt[k * 8 + r]);
  jpeg_idct8(v, 11);
}

// The decoded planes a pixel is made of: 8-bit Y' and (C = 3) Cb', Cr' with their pitches; (y0, x0) is the picture
// position of yp's first sample and (cy0, cx0) the position of the chroma planes' first sample in chroma coordinates.
struct JpegDec {
  const uint8_t *yp, *cbp, *crp;
  int ypitch, cpitch, y0, x0, cy0, cx0;
};

// libjpeg's "fancy" triangle filter at pixel (y, x) over the ceil(H/2) x ceil(W/2) real samples of a decoded chroma
// plane.  libjpeg takes it only for planes wider than two samples; narrower ones are replicated.
__host__ __device__ __forceinline__ int jpeg_fancy(const JpegPic& p, const JpegDec& d, const uint8_t* c, int y, int x) {
  const int ch = (p.H + 1) >> 1, cw = (p.W + 1) >> 1, i = y >> 1, j = x >> 1;
  const ptrdiff_t row = (ptrdiff_t)(i - d.cy0) * d.cpitch - d.cx0;      // + j: the sample's index in the plane
  if (cw <= 2) return c[row + j];
  const int i2 = jpeg_clamp((y & 1) ? i + 1 : i - 1, 0, ch - 1), j2 = jpeg_clamp((x & 1) ? j + 1 : j - 1, 0, cw - 1);
  const ptrdiff_t row2 = (ptrdiff_t)(i2 - d.cy0) * d.cpitch - d.cx0;
  const int s = 3 * c[row + j] + c[row2 + j], s2 = 3 * c[row + j2] + c[row2 + j2];
  return (3 * s + s2 + ((x & 1) ? 7 : 8)) >> 4;
}

// The picture's pixel (y, x) from the decoded planes: chroma back to full size, then the colour tail.
__host__ __device__ __forceinline__ void jpeg_pixel(const JpegPic& p, const JpegDec& d, int y, int x, int out[3]) {
  const int Y = d.yp[(size_t)(y - d.y0) * d.ypitch + (x - d.x0)];
  out[0] = Y;
  if (p.C == 1) return;
  int cb, cr;
  if (p.sub) {
    cb = jpeg_fancy(p, d, d.cbp, y, x);
    cr = jpeg_fancy(p, d, d.crp, y, x);
  } else {
    const size_t o = (size_t)(y - d.cy0) * d.cpitch + (x - d.cx0);
    cb = d.cbp[o];
    cr = d.crp[o];
  }
  if (!p.color) {
    out[1] = cb;
    out[2] = cr;
    return;
  }
  cb -= 128;
  cr -= 128;
  out[0] = jpeg_clamp(Y + ((91881 * cr + 32768) >> 16), 0, 255);
  out[1] = jpeg_clamp(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);
  out[2] = jpeg_clamp(Y + ((116130 * cb + 32768) >> 16), 0, 255);
}

}  // namespace srk
#endif  // SRK_JPEG_COMMON_H_
