// JPEG artefacts on the loader's 8-bit patches: y = decode(encode(x, Q)) per patch, byte for byte what libjpeg's baseline
// integer path gives (jpeg_common.h holds the definition; include/srk.h).
//
// k_jpeg_u8: a block of 256 threads owns a 64 x 64 pixel tile of one picture, every component of it.  Eight lanes take one
// 8 x 8 block: lane r samples row r from global memory (colour conversion, chroma shrink and edge replication are part of
// the fetch), makes the forward row pass, hands the block through LDS to the lane of column r (rows of 9 dwords: both the
// row writes and the column reads touch 32 different banks per half wave), which makes the forward column pass, the
// quantisation and the inverse column pass in registers, and hands it back for the inverse row pass.  The decoded 8-bit
// planes of the tile stay in LDS.  With 4:2:0 the triangle upsampling reads one chroma sample beyond the tile, so the
// block also decodes the ring of chroma blocks around its own 4 x 4 -- where the picture has such blocks: a picture of
// one tile (the 32 x 32 training patch) has none.  Then every thread makes runs of four output pixels from the planes.
// A patch of quality 0 skips all of it and is copied.
#include <vector>
#include "srk_common.h"
#include "jpeg_common.h"

namespace srk {

constexpr int kJpegTile = 64;                      // pixels per tile side: 8 luma blocks, 4 (+ 2 ring) 4:2:0 chroma blocks
constexpr int kJpegPitch = 9;                      // dwords per row of a group's 8 x 8 exchange buffer
constexpr int kJpegSubPitch = kJpegTile / 2 + 16;  // bytes per row of a 4:2:0 chroma plane with its ring: 6 blocks
static_assert(kJpegSubPitch * kJpegSubPitch <= kJpegTile * kJpegTile && kJpegSubPitch % 4 == 0,
              "a ringed chroma plane fits the space of a full-size one and its rows start on a dword");

__device__ __forceinline__ void jpeg_store4(uint8_t* y, const int* v, int n, bool vec) {
  if (vec) {
    *reinterpret_cast<uint32_t*>(y) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
  } else {
#pragma unroll
    for (int o = 0; o < 4; ++o)
      if (o < n) y[o] = (uint8_t)v[o];
  }
}

__device__ __forceinline__ void jpeg_store4(float* y, const int* v, int n, bool vec) {
  if (vec) {
    f32x4 o = {(float)v[0] / 255.f, (float)v[1] / 255.f, (float)v[2] / 255.f, (float)v[3] / 255.f};
    *reinterpret_cast<f32x4*>(y) = o;
  } else {
#pragma unroll
    for (int o = 0; o < 4; ++o)
      if (o < n) y[o] = (float)v[o] / 255.f;
  }
}

template <typename OutT>
__global__ __launch_bounds__(256) void k_jpeg_u8(const uint8_t* __restrict__ x, OutT* __restrict__ y,
                                                 const double* __restrict__ quality, int C, int H, int W, int sub, int color,
                                                 int tiles_x, int tiles_per_pic) {
  __shared__ int sT[32 * 8 * kJpegPitch];
  __shared__ int sQ[2 * 64];
  __shared__ uint32_t sDec[3][kJpegTile * kJpegTile / 4];

  const int b = blockIdx.x / tiles_per_pic, t = blockIdx.x - b * tiles_per_pic;
  const int ty0 = (t / tiles_x) * kJpegTile, tx0 = (t % tiles_x) * kJpegTile;
  const size_t pic_elems = (size_t)C * H * W;
  const JpegPic pic = {x + b * pic_elems, C, H, W, sub, color};
  const int Q = (int)quality[b];

  // (first block, blocks) of the tile per direction: luma, and chroma with its ring clipped to the blocks that hold real
  // samples.  c*_nom is the block that local block 0 of the chroma planes stands for, inside the picture or not.
  const int ly0 = ty0 / 8, lx0 = tx0 / 8;
  const int lny = jpeg_min(8, (H + 7) / 8 - ly0), lnx = jpeg_min(8, (W + 7) / 8 - lx0);
  const int cy_nom = sub ? ty0 / 16 - 1 : ly0, cx_nom = sub ? tx0 / 16 - 1 : lx0;
  const int cpitch = sub ? kJpegSubPitch : kJpegTile;
  int cy_lo = ly0, cx_lo = lx0, cny = lny, cnx = lnx;
  if (sub) {
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    cy_lo = cy_nom < 0 ? 0 : cy_nom;
    cx_lo = cx_nom < 0 ? 0 : cx_nom;
    cny = jpeg_min((ch + 7) / 8 - 1, cy_nom + 5) - cy_lo + 1;
    cnx = jpeg_min((cw + 7) / 8 - 1, cx_nom + 5) - cx_lo + 1;
  }

  if (Q != 0) {
    if (threadIdx.x < 128) sQ[threadIdx.x] = jpeg_quant(Q, threadIdx.x >> 6, threadIdx.x & 63);
    const int luma_jobs = lny * lnx, chroma_jobs = C == 3 ? cny * cnx : 0, jobs = luma_jobs + 2 * chroma_jobs;
    const int g = threadIdx.x >> 3, r = threadIdx.x & 7;
    int* T = sT + g * (8 * kJpegPitch);
    __syncthreads();
    for (int job0 = 0; job0 < jobs; job0 += 32) {          // (the same trips for every thread: the barriers below)
      const int job = job0 + g;
      const bool active = job < jobs;
      int comp = 0, bi = 0, bj = 0, lrow = 0, lcol = 0, pitch = kJpegTile;
      if (active) {
        if (job < luma_jobs) {
          bi = ly0 + job / lnx, bj = lx0 + job % lnx;
          lrow = (bi - ly0) * 8, lcol = (bj - lx0) * 8;
        } else {
          const int cj = job - luma_jobs;
          comp = 1 + cj / chroma_jobs;
          const int k = cj % chroma_jobs;
          bi = cy_lo + k / cnx, bj = cx_lo + k % cnx;
          lrow = (bi - cy_nom) * 8, lcol = (bj - cx_nom) * 8, pitch = cpitch;
        }
      }
      int v[8];
      if (active) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = jpeg_sample(pic, comp, bi * 8 + r, bj * 8 + k) - 128;
        jpeg_fdct8(v, true);
#pragma unroll
        for (int k = 0; k < 8; ++k) T[r * kJpegPitch + k] = v[k];
      }
      __syncthreads();
      if (active) {      // column r: lane r reads and then rewrites only its own column
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = T[k * kJpegPitch + r];
        jpeg_block_column(v, sQ + (comp ? 64 : 0), r);
#pragma unroll
        for (int k = 0; k < 8; ++k) T[k * kJpegPitch + r] = v[k];
      }
      __syncthreads();
      if (active) {      // row r again (the next trip's row write is this lane's own row too)
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = T[r * kJpegPitch + k];
        jpeg_idct8(v, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          lo |= (uint32_t)jpeg_clamp(v[k] + 128, 0, 255) << (8 * k);
          hi |= (uint32_t)jpeg_clamp(v[k + 4] + 128, 0, 255) << (8 * k);
        }
        uint32_t* dst = sDec[comp] + ((lrow + r) * pitch + lcol) / 4;
        dst[0] = lo;
        dst[1] = hi;
      }
    }
    __syncthreads();
  }

  const JpegDec dec = {reinterpret_cast<const uint8_t*>(sDec[0]), reinterpret_cast<const uint8_t*>(sDec[1]),
                       reinterpret_cast<const uint8_t*>(sDec[2]), kJpegTile, cpitch, ty0, tx0,
                       sub ? cy_nom * 8 : ty0, sub ? cx_nom * 8 : tx0};
  OutT* yb = y + b * pic_elems;
  const size_t plane = (size_t)H * W;
  for (int idx = threadIdx.x; idx < kJpegTile * kJpegTile / 4; idx += 256) {
    const int py = ty0 + idx / (kJpegTile / 4), px = tx0 + (idx % (kJpegTile / 4)) * 4;
    if (py >= H || px >= W) continue;
    const int n = jpeg_min(4, W - px);
    int o[3][4] = {};
#pragma unroll          // (whole unrolling keeps o[][] in registers)
    for (int k = 0; k < 4; ++k) {
      if (k >= n) break;
      int p3[3] = {0, 0, 0};
      if (Q != 0) {
        jpeg_pixel(pic, dec, py, px + k, p3);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (c < C) p3[c] = pic.x[c * plane + (size_t)py * W + px + k];
      }
      o[0][k] = p3[0], o[1][k] = p3[1], o[2][k] = p3[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c >= C) break;
      OutT* yp = yb + c * plane + (size_t)py * W + px;
      jpeg_store4(yp, o[c], n, n == 4 && (reinterpret_cast<uintptr_t>(yp) & (4 * sizeof(OutT) - 1)) == 0);
    }
  }
}

// The whole round trip of one picture on the host: the blocks of every component in turn through the very bodies the kernel
// compiles, the decoded planes whole in memory, then every pixel.
static void jpeg_picture_host(const JpegPic& pic, uint8_t* y, int Q) {
  const int H = pic.H, W = pic.W, C = pic.C;
  const size_t plane = (size_t)H * W;
  if (Q == 0) {
    for (size_t e = 0; e < plane * C; ++e) y[e] = pic.x[e];
    return;
  }
  int qt[2][64];
  for (int c = 0; c < 2; ++c)
    for (int k = 0; k < 64; ++k) qt[c][k] = jpeg_quant(Q, c, k);
  std::vector<uint8_t> dec[3];
  int pitch[3] = {0, 0, 0};
  for (int comp = 0; comp < C; ++comp) {
    const bool small = comp > 0 && pic.sub;
    const int h = small ? (H + 1) >> 1 : H, w = small ? (W + 1) >> 1 : W, nby = (h + 7) / 8, nbx = (w + 7) / 8;
    pitch[comp] = nbx * 8;
    dec[comp].resize((size_t)nby * 8 * nbx * 8);
    for (int bi = 0; bi < nby; ++bi)
      for (int bj = 0; bj < nbx; ++bj) {
        int blk[8][8], v[8];
        for (int r = 0; r < 8; ++r) {
          for (int k = 0; k < 8; ++k) blk[r][k] = jpeg_sample(pic, comp, bi * 8 + r, bj * 8 + k) - 128;
          jpeg_fdct8(blk[r], true);
        }
        for (int r = 0; r < 8; ++r) {
          for (int k = 0; k < 8; ++k) v[k] = blk[k][r];
          jpeg_block_column(v, qt[comp ? 1 : 0], r);
          for (int k = 0; k < 8; ++k) blk[k][r] = v[k];
        }
        for (int r = 0; r < 8; ++r) {
          jpeg_idct8(blk[r], 18);
          for (int k = 0; k < 8; ++k)
            dec[comp][(size_t)(bi * 8 + r) * pitch[comp] + bj * 8 + k] = (uint8_t)jpeg_clamp(blk[r][k] + 128, 0, 255);
        }
      }
  }
  const JpegDec d = {dec[0].data(), dec[1].data(), dec[2].data(), pitch[0], pitch[1], 0, 0, 0, 0};
  for (int py = 0; py < H; ++py)
    for (int px = 0; px < W; ++px) {
      int p3[3] = {0, 0, 0};
      jpeg_pixel(pic, d, py, px, p3);
      for (int c = 0; c < C; ++c) y[c * plane + (size_t)py * W + px] = (uint8_t)p3[c];
    }
}

}  // namespace srk

using namespace srk;

#define SRK_JPEG_REQUIRE_SHAPE(what)                                                                                      \
  SRK_REQUIRE(C == 1 || C == 3, what ": C must be 1 or 3 (got %d)", C);                                                  \
  SRK_REQUIRE(B > 0 && H > 0 && W > 0, what ": bad dims (B %d, %d x %d)", B, H, W);                                      \
  SRK_REQUIRE(subsampling == 0 || subsampling == 1, what ": subsampling must be 0 (4:4:4) or 1 (4:2:0), got %d",         \
              subsampling);                                                                                               \
  SRK_REQUIRE(color == 0 || (color == 1 && C == 3), what ": color must be 0 or 1, and 1 needs C = 3 (got color %d, C %d)", \
              color, C)

extern "C" int srk_jpeg_u8(const uint8_t* x, void* y, const double* quality, int C, int B, int H, int W, int subsampling,
                           int color, int out_float, void* stream) {
  SRK_REQUIRE(x && y && quality, "jpeg_u8: null pointer");
  SRK_JPEG_REQUIRE_SHAPE("jpeg_u8");
  const int tiles_x = (W + kJpegTile - 1) / kJpegTile, tiles_y = (H + kJpegTile - 1) / kJpegTile;
  const int64_t blocks = (int64_t)B * tiles_x * tiles_y;
  SRK_REQUIRE(blocks <= 0x7fffffff, "jpeg_u8: %lld tiles are more than one launch takes", (long long)blocks);
  const int sub = C == 3 ? subsampling : 0;
  hipStream_t s = (hipStream_t)stream;
  if (out_float)
    hipLaunchKernelGGL(k_jpeg_u8<float>, dim3((unsigned)blocks), dim3(256), 0, s, x, static_cast<float*>(y), quality, C, H, W,
                       sub, color, tiles_x, tiles_x * tiles_y);
  else
    hipLaunchKernelGGL(k_jpeg_u8<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, s, x, static_cast<uint8_t*>(y), quality, C, H,
                       W, sub, color, tiles_x, tiles_x * tiles_y);
  return check_launch("jpeg_u8");
}

extern "C" int srk_jpeg_quant_table_host(int quality, int chroma, int* out) {
  SRK_REQUIRE(out, "jpeg_quant_table_host: null pointer");
  SRK_REQUIRE(chroma == 0 || chroma == 1, "jpeg_quant_table_host: chroma must be 0 or 1 (got %d)", chroma);
  for (int k = 0; k < 64; ++k) out[k] = jpeg_quant(quality, chroma, k);
  return SRK_OK;
}

extern "C" int srk_jpeg_u8_host(const uint8_t* x, uint8_t* y, const int* quality, int C, int B, int H, int W, int subsampling,
                                int color) {
  SRK_REQUIRE(x && y && quality, "jpeg_u8_host: null pointer");
  SRK_JPEG_REQUIRE_SHAPE("jpeg_u8_host");
  const size_t pic_elems = (size_t)C * H * W;
  for (int b = 0; b < B; ++b) {
    const JpegPic pic = {x + b * pic_elems, C, H, W, C == 3 ? subsampling : 0, color};
    jpeg_picture_host(pic, y + b * pic_elems, quality[b]);
  }
  return SRK_OK;
}
