// Tiled super-resolution of one picture (tiling.py): cut the net's input into the equal, overlapping tiles of a plan
// (k_tile_gather) and put the tiles' outputs back together, every output pixel from the ONE tile that owns it
// (k_tile_stitch) -- as the fp32 picture, or straight as the final interleaved 8-bit picture (quantised like k_to_u8, or
// quantised and converted with 8-bit chroma planes like k_ycc_to_rgb: the fp32 HR picture is then never written).
//
// The plan is separable, so the device table is one entry per tile ROW and one per tile COLUMN, rows first:
//     int32 {in0, own0, own1, out0}:  input offset of the tile, [own0, own1) the output pixels it owns, out0 the output
//                                     pixel of the tile's local output pixel 0 (= scale * in0)
// Tile t = row * ntx + col; a call handles the tiles t0 .. t0 + n of the plan (one chunk of the batch loop).
//
// Access pattern of color.hip: a thread owns a run of 16 DESTINATION pixels of the flat pixel sequence, so every run of
// a dense destination starts 16-byte aligned whatever the width, every access is 16 bytes wide where pointer and run
// allow and scalar otherwise (decided per pointer), and every destination byte is written exactly once: no atomics, no
// scratch.  What is new here is a run that is not one stretch of one source row: it crosses an ownership boundary
// between two tile columns, or the end of a destination row.  Such a run is walked pixel by pixel (row, column and
// owning tile advance incrementally); a run that lies in one row of one tile takes the wide path.  A chunk writes only
// the pixels its own tiles own, so the chunks of a picture together write it once.
//
// The table lives in device memory and the host never reads it back, so the kernels do not trust it: a local coordinate
// outside the tile (or a source pixel outside the picture) is skipped, never dereferenced.
#include "color_common.h"

namespace srk {

struct TileAxis { int in0, own0, own1, out0; };

// the entry of `ax[0..n)` that owns destination pixel o, or -1
__device__ __forceinline__ int tile_owner(const TileAxis* __restrict__ ax, int n, int o) {
  for (int i = 0; i < n; ++i)
    if (o >= ax[i].own0 && o < ax[i].own1) return i;
  return -1;
}

// fp32 picture [C][H][W] through element strides -> dense NHWC tiles [n][th][tw][C].  Runs are over the flat destination
// pixel sequence (tile, y, x): 16 pixels = 16 C consecutive floats.
template <int C>
__global__ __launch_bounds__(256) void k_tile_gather(const float* __restrict__ pic, long long sc, long long sh, long long sw,
                                                     int H, int W, const TileAxis* __restrict__ tab, int nty, int ntx, int th,
                                                     int tw, int t0, int n, float* __restrict__ out) {
  const TileAxis* rows = tab;
  const TileAxis* cols = tab + nty;
  const size_t per_tile = (size_t)th * tw;
  const size_t total = per_tile * (size_t)n;
  const size_t runs = (total + kRun - 1) / kRun;
  for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < runs; r += (size_t)gridDim.x * 256) {
    const size_t p0 = r * kRun;
    const int nrun = total - p0 < (size_t)kRun ? (int)(total - p0) : kRun;
    int tile = (int)(p0 / per_tile);
    const size_t rem = p0 - (size_t)tile * per_tile;
    int y = (int)(rem / tw), x = (int)(rem - (size_t)y * tw);
    float v[C][kRun];
    if (x + nrun <= tw) {   // one stretch of one picture row
      const int t = t0 + tile;
      const int iy = rows[t / ntx].in0 + y, ix = cols[t % ntx].in0 + x;
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix + nrun <= W;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        if (ok) {
          load_floats(pic + c * sc + (long long)iy * sh + (long long)ix * sw, sw, nrun, v[c]);
        } else {
#pragma unroll
          for (int k = 0; k < kRun; ++k) v[c][k] = 0.f;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        const int t = t0 + tile;
        const int iy = rows[t / ntx].in0 + y, ix = cols[t % ntx].in0 + x;
        const bool ok = k < nrun && iy >= 0 && iy < H && ix >= 0 && ix < W;
#pragma unroll
        for (int c = 0; c < C; ++c) v[c][k] = ok ? pic[c * sc + (long long)iy * sh + (long long)ix * sw] : 0.f;
        if (++x == tw) {
          x = 0;
          if (++y == th) y = 0, tile = tile + 1 < n ? tile + 1 : tile;   // (past the last tile only beyond nrun)
        }
      }
    }
    float* d = out + p0 * C;
    if (nrun == kRun && aligned16(d)) {
#pragma unroll
      for (int q = 0; q < 4 * C; ++q) {
        const int e = 4 * q;   // element e of the run's 16 C floats is pixel e / C, channel e % C
        reinterpret_cast<float4*>(d)[q] = make_float4(v[e % C][e / C], v[(e + 1) % C][(e + 1) / C], v[(e + 2) % C][(e + 2) / C],
                                                      v[(e + 3) % C][(e + 3) / C]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kRun; ++k)
        if (k < nrun) {
#pragma unroll
          for (int c = 0; c < C; ++c) d[k * C + c] = v[c][k];
        }
    }
  }
}

// MODE of the stitch's destination
constexpr int kStitchF32 = 0;   // fp32 planar [C][OH][OW]
constexpr int kStitchU8 = 1;    // interleaved 8-bit [OH][OW][C], quantised like k_to_u8
constexpr int kStitchYcc = 2;   // C = 1: Y quantised, + 8-bit Cb / Cr planes [OH][OW] -> interleaved RGB like k_ycc_to_rgb

// tile outputs [n][C][oth][otw] through element strides -> the picture.  Runs are over the flat destination pixel
// sequence of the rows the chunk's tile rows own.
template <int C, int MODE>
__global__ __launch_bounds__(256) void k_tile_stitch(const float* __restrict__ src, long long sn, long long sc, long long sh,
                                                     long long sw, int oth, int otw, const TileAxis* __restrict__ tab, int nty,
                                                     int ntx, int t0, int n, float* __restrict__ out_f32,
                                                     unsigned char* __restrict__ out_u8, const unsigned char* __restrict__ cb,
                                                     const unsigned char* __restrict__ cr, int OH, int OW) {
  constexpr int OC = MODE == kStitchYcc ? 3 : C;   // channels of the 8-bit destination
  __shared__ alignas(16) int16_t ctab[MODE == kStitchYcc ? kInvTabs * 256 : 8];
  if (MODE == kStitchYcc) stage_tables<kInvTabs>(kColorDev.inv, ctab);
  const TileAxis* rows = tab;
  const TileAxis* cols = tab + nty;
  const int ty_first = t0 / ntx, ty_last = (t0 + n - 1) / ntx;
  int row0 = rows[ty_first].own0, row1 = rows[ty_last].own1;
  row0 = row0 < 0 ? 0 : row0;
  row1 = row1 > OH ? OH : row1;
  if (row1 <= row0) return;
  const size_t plane = (size_t)OH * OW;
  const size_t r_begin = (size_t)row0 * OW / kRun, r_end = ((size_t)row1 * OW + kRun - 1) / kRun;
  for (size_t r = r_begin + (size_t)blockIdx.x * 256 + threadIdx.x; r < r_end; r += (size_t)gridDim.x * 256) {
    const size_t p0 = r * kRun;
    const int nrun = plane - p0 < (size_t)kRun ? (int)(plane - p0) : kRun;
    int Y = (int)(p0 / OW), X = (int)(p0 - (size_t)Y * OW);
    int ty = tile_owner(rows, nty, Y), tx = tile_owner(cols, ntx, X);
    float v[C][kRun];
    unsigned own = 0;   // bit k: pixel k of the run is owned by a tile of this chunk
    if (ty >= 0 && tx >= 0 && X + nrun <= OW && X + nrun <= cols[tx].own1) {   // one stretch of one tile row
      const int t = ty * ntx + tx;
      const int ly = Y - rows[ty].out0, lx = X - cols[tx].out0;
      if (t < t0 || t >= t0 + n || ly < 0 || ly >= oth || lx < 0 || lx + nrun > otw) continue;
      const float* s = src + (long long)(t - t0) * sn + (long long)ly * sh + (long long)lx * sw;
      if (C == 3 && sc == 1 && sw == 3 && nrun == kRun && aligned16(s)) {   // channels-last: 48 consecutive floats
#pragma unroll
        for (int q = 0; q < 12; ++q) {
          const float4 f = reinterpret_cast<const float4*>(s)[q];
          const int e = 4 * q;
          v[e % C][e / C] = f.x, v[(e + 1) % C][(e + 1) / C] = f.y, v[(e + 2) % C][(e + 2) / C] = f.z,
                       v[(e + 3) % C][(e + 3) / C] = f.w;
        }
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) load_floats(s + c * sc, sw, nrun, v[c]);
      }
      own = nrun == kRun ? 0xffffu : (1u << nrun) - 1u;
    } else {
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        bool ok = k < nrun && ty >= 0 && tx >= 0;
        if (ok) {
          const int t = ty * ntx + tx;
          const int ly = Y - rows[ty].out0, lx = X - cols[tx].out0;
          ok = t >= t0 && t < t0 + n && ly >= 0 && ly < oth && lx >= 0 && lx < otw;
          if (ok) {
            const float* s = src + (long long)(t - t0) * sn + (long long)ly * sh + (long long)lx * sw;
#pragma unroll
            for (int c = 0; c < C; ++c) v[c][k] = s[c * sc];
            own |= 1u << k;
          }
        }
        if (!ok) {
#pragma unroll
          for (int c = 0; c < C; ++c) v[c][k] = 0.f;
        }
        if (++X == OW) {   // the run goes on in the next destination row
          X = 0, ++Y;
          tx = tile_owner(cols, ntx, 0);
          if (ty < 0 || Y >= rows[ty].own1) ty = tile_owner(rows, nty, Y);
        } else if (tx < 0 || X >= cols[tx].own1) {   // ... or in the next tile column
          tx = tile_owner(cols, ntx, X);
        }
      }
      if (!own) continue;
    }
    const bool all = own == 0xffffu;
    if (MODE == kStitchF32) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float* d = out_f32 + c * plane + p0;
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
      if (MODE == kStitchU8) {
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
          for (int k = 0; k < kRun; ++k) {
            const int b = k * C + c;
            w[b >> 2] |= quant_u8(v[c][k]) << ((b & 3) * 8);
          }
      } else {
        unsigned bw[4], rw[4];
        load_bytes<4>(cb + p0, nrun == kRun && aligned16(cb + p0), nrun, bw);
        load_bytes<4>(cr + p0, nrun == kRun && aligned16(cr + p0), nrun, rw);
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
          int rr, gg, bb;
          ycc_to_rgb_px(ctab, (int)quant_u8(v[0][k]), (int)get_byte(bw, k), (int)get_byte(rw, k), rr, gg, bb);
          w[(3 * k) >> 2] |= (unsigned)rr << (((3 * k) & 3) * 8);
          w[(3 * k + 1) >> 2] |= (unsigned)gg << (((3 * k + 1) & 3) * 8);
          w[(3 * k + 2) >> 2] |= (unsigned)bb << (((3 * k + 2) & 3) * 8);
        }
      }
      unsigned char* d = out_u8 + p0 * OC;
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
}

static dim3 flat_grid(size_t pixels) {
  const size_t nb = ((pixels + kRun - 1) / kRun + 255) / 256;
  return dim3((unsigned)(nb > 65535 ? 65535 : (nb < 1 ? 1 : nb)));
}

static int stitch_args_ok(const char* what, const void* tiles, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int C, int oth,
                          int otw, const void* table, int nty, int ntx, int t0, int n, const void* out, int OH, int OW) {
  SRK_REQUIRE(tiles && table && out, "%s: null pointer", what);
  SRK_REQUIRE(C == 1 || C == 3, "%s: C must be 1 or 3 (got %d)", what, C);
  SRK_REQUIRE(oth > 0 && otw > 0 && OH > 0 && OW > 0, "%s: non-positive dims (tile %d x %d, picture %d x %d)", what, oth, otw,
              OH, OW);
  SRK_REQUIRE(oth <= OH && otw <= OW, "%s: a tile output of %d x %d is larger than the picture %d x %d", what, oth, otw, OH, OW);
  SRK_REQUIRE(sn >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "%s: negative strides", what);
  SRK_REQUIRE(nty > 0 && ntx > 0 && nty <= 32768 && ntx <= 32768, "%s: bad plan (%d x %d tiles)", what, nty, ntx);
  SRK_REQUIRE(n > 0 && t0 >= 0 && (long long)t0 + n <= (long long)nty * ntx, "%s: tiles %d .. %d are not in a plan of %d x %d", what,
              t0, t0 + n, nty, ntx);
  return SRK_OK;
}

// the rows a chunk can own are not known to the host (the table is on the device): size the grid for rows of whole tile
// rows, an upper bound of what the kernel walks
static dim3 stitch_grid(int oth, int OH, int OW, int ntx, int t0, int n) {
  const long long tile_rows = (long long)(t0 + n - 1) / ntx - t0 / ntx + 1;
  long long rows = tile_rows * oth;
  if (rows > OH) rows = OH;
  return flat_grid((size_t)rows * OW);
}

}  // namespace srk

using namespace srk;

extern "C" int srk_tile_gather(const float* pic, int64_t c_stride, int64_t row_stride, int64_t px_stride, int C, int H, int W,
                               const int32_t* table, int nty, int ntx, int th, int tw, int t0, int n, float* out, void* stream) {
  SRK_REQUIRE(pic && table && out, "tile_gather: null pointer");
  SRK_REQUIRE(C == 1 || C == 3, "tile_gather: C must be 1 or 3 (got %d)", C);
  SRK_REQUIRE(H > 0 && W > 0 && th > 0 && tw > 0 && th <= H && tw <= W, "tile_gather: tiles of %d x %d do not fit a picture of %d x %d",
              th, tw, H, W);
  SRK_REQUIRE(c_stride >= 0 && row_stride >= 0 && px_stride >= 0, "tile_gather: negative strides");
  SRK_REQUIRE(nty > 0 && ntx > 0 && nty <= 32768 && ntx <= 32768, "tile_gather: bad plan (%d x %d tiles)", nty, ntx);
  SRK_REQUIRE(n > 0 && t0 >= 0 && (long long)t0 + n <= (long long)nty * ntx, "tile_gather: tiles %d .. %d are not in a plan of %d x %d",
              t0, t0 + n, nty, ntx);
  const dim3 grid = flat_grid((size_t)n * th * tw);
  const TileAxis* tab = reinterpret_cast<const TileAxis*>(table);
  if (C == 3)
    hipLaunchKernelGGL(k_tile_gather<3>, grid, dim3(256), 0, (hipStream_t)stream, pic, (long long)c_stride, (long long)row_stride,
                       (long long)px_stride, H, W, tab, nty, ntx, th, tw, t0, n, out);
  else
    hipLaunchKernelGGL(k_tile_gather<1>, grid, dim3(256), 0, (hipStream_t)stream, pic, (long long)c_stride, (long long)row_stride,
                       (long long)px_stride, H, W, tab, nty, ntx, th, tw, t0, n, out);
  return check_launch("tile_gather");
}

extern "C" int srk_tile_stitch_f32(const float* tiles, int64_t n_stride, int64_t c_stride, int64_t row_stride, int64_t px_stride,
                                   int C, int oth, int otw, const int32_t* table, int nty, int ntx, int t0, int n, float* out,
                                   int OH, int OW, void* stream) {
  const int rc = stitch_args_ok("tile_stitch_f32", tiles, n_stride, c_stride, row_stride, px_stride, C, oth, otw, table, nty, ntx,
                                t0, n, out, OH, OW);
  if (rc != SRK_OK) return rc;
  const dim3 grid = stitch_grid(oth, OH, OW, ntx, t0, n);
  const TileAxis* tab = reinterpret_cast<const TileAxis*>(table);
  if (C == 3)
    hipLaunchKernelGGL((k_tile_stitch<3, kStitchF32>), grid, dim3(256), 0, (hipStream_t)stream, tiles, (long long)n_stride,
                       (long long)c_stride, (long long)row_stride, (long long)px_stride, oth, otw, tab, nty, ntx, t0, n, out,
                       (unsigned char*)nullptr, (const unsigned char*)nullptr, (const unsigned char*)nullptr, OH, OW);
  else
    hipLaunchKernelGGL((k_tile_stitch<1, kStitchF32>), grid, dim3(256), 0, (hipStream_t)stream, tiles, (long long)n_stride,
                       (long long)c_stride, (long long)row_stride, (long long)px_stride, oth, otw, tab, nty, ntx, t0, n, out,
                       (unsigned char*)nullptr, (const unsigned char*)nullptr, (const unsigned char*)nullptr, OH, OW);
  return check_launch("tile_stitch_f32");
}

extern "C" int srk_tile_stitch_u8(const float* tiles, int64_t n_stride, int64_t c_stride, int64_t row_stride, int64_t px_stride,
                                  int C, int oth, int otw, const int32_t* table, int nty, int ntx, int t0, int n,
                                  const uint8_t* cb, const uint8_t* cr, uint8_t* out, int OH, int OW, void* stream) {
  const int rc = stitch_args_ok("tile_stitch_u8", tiles, n_stride, c_stride, row_stride, px_stride, C, oth, otw, table, nty, ntx,
                                t0, n, out, OH, OW);
  if (rc != SRK_OK) return rc;
  SRK_REQUIRE((cb != nullptr) == (cr != nullptr), "tile_stitch_u8: cb and cr come together");
  SRK_REQUIRE(!cb || C == 1, "tile_stitch_u8: chroma planes go with a Y output (C = 1), got C = %d", C);
  const dim3 grid = stitch_grid(oth, OH, OW, ntx, t0, n);
  const TileAxis* tab = reinterpret_cast<const TileAxis*>(table);
  const long long sn = n_stride, sc = c_stride, sh = row_stride, sw = px_stride;
  if (cb)
    hipLaunchKernelGGL((k_tile_stitch<1, kStitchYcc>), grid, dim3(256), 0, (hipStream_t)stream, tiles, sn, sc, sh, sw, oth, otw,
                       tab, nty, ntx, t0, n, (float*)nullptr, out, cb, cr, OH, OW);
  else if (C == 3)
    hipLaunchKernelGGL((k_tile_stitch<3, kStitchU8>), grid, dim3(256), 0, (hipStream_t)stream, tiles, sn, sc, sh, sw, oth, otw,
                       tab, nty, ntx, t0, n, (float*)nullptr, out, (const unsigned char*)nullptr, (const unsigned char*)nullptr,
                       OH, OW);
  else
    hipLaunchKernelGGL((k_tile_stitch<1, kStitchU8>), grid, dim3(256), 0, (hipStream_t)stream, tiles, sn, sc, sh, sw, oth, otw,
                       tab, nty, ntx, t0, n, (float*)nullptr, out, (const unsigned char*)nullptr, (const unsigned char*)nullptr,
                       OH, OW);
  return check_launch("tile_stitch_u8");
}
