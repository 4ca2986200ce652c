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
__global__ __launch_bounds__(256) void k_tile_gather(const float* __restrict__ pic, Strides4 s, int H, int W,
                                                     const TileAxis* __restrict__ tab, int nty, int ntx, int th, int tw, int t0,
                                                     int n, float* __restrict__ out) {
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
      if (ok) {
        load_planes<C>(pic + (long long)iy * s.h + (long long)ix * s.w, s.c, s.w, nrun, v);
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
          for (int k = 0; k < kRun; ++k) v[c][k] = 0.f;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        const int t = t0 + tile;
        const int iy = rows[t / ntx].in0 + y, ix = cols[t % ntx].in0 + x;
        const bool ok = k < nrun && iy >= 0 && iy < H && ix >= 0 && ix < W;
#pragma unroll
        for (int c = 0; c < C; ++c) v[c][k] = ok ? pic[c * s.c + (long long)iy * s.h + (long long)ix * s.w] : 0.f;
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

// tile outputs [n][C][oth][otw] through element strides -> the picture.  Runs are over the flat destination pixel
// sequence of the rows the chunk's tile rows own; DST (kDstF32 / kDstU8 / kDstYcc) is what store_run makes of them.
template <int C, int DST>
__global__ __launch_bounds__(256) void k_tile_stitch(const float* __restrict__ src, Strides4 ss, int oth, int otw,
                                                     const TileAxis* __restrict__ tab, int nty, int ntx, int t0, int n,
                                                     PicDst dst, int OH, int OW) {
  __shared__ alignas(16) int16_t ctab[DST == kDstYcc ? kInvTabs * 256 : 8];
  if (DST == kDstYcc) stage_tables<kInvTabs>(kColorDev.inv, ctab);
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
      load_run<C>(src + (long long)(t - t0) * ss.n + (long long)ly * ss.h + (long long)lx * ss.w, ss.c, ss.w, nrun, v);
      own = run_mask(nrun);
    } else {
#pragma unroll
      for (int k = 0; k < kRun; ++k) {
        bool ok = k < nrun && ty >= 0 && tx >= 0;
        if (ok) {
          const int t = ty * ntx + tx;
          const int ly = Y - rows[ty].out0, lx = X - cols[tx].out0;
          ok = t >= t0 && t < t0 + n && ly >= 0 && ly < oth && lx >= 0 && lx < otw;
          if (ok) {
            const float* s = src + (long long)(t - t0) * ss.n + (long long)ly * ss.h + (long long)lx * ss.w;
#pragma unroll
            for (int c = 0; c < C; ++c) v[c][k] = s[c * ss.c];
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
    store_run<C, DST>(v, own, nrun, p0, plane, dst, ctab);
  }
}

static dim3 flat_grid(size_t pixels) { return run_grid((pixels + kRun - 1) / kRun); }

static int stitch_args_ok(const char* what, const void* tiles, const Strides4& s, int C, int oth, int otw, const void* table,
                          int nty, int ntx, int t0, int n, const void* out, int OH, int OW) {
  SRK_REQUIRE(tiles && table && out, "%s: null pointer", what);
  SRK_REQUIRE(C == 1 || C == 3, "%s: C must be 1 or 3 (got %d)", what, C);
  SRK_REQUIRE(oth > 0 && otw > 0 && OH > 0 && OW > 0, "%s: non-positive dims (tile %d x %d, picture %d x %d)", what, oth, otw,
              OH, OW);
  SRK_REQUIRE(oth <= OH && otw <= OW, "%s: a tile output of %d x %d is larger than the picture %d x %d", what, oth, otw, OH, OW);
  SRK_REQUIRE(s.n >= 0 && s.c >= 0 && s.h >= 0 && s.w >= 0, "%s: negative strides", what);
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
  launch_pic(C, kDstF32, [&](auto c, auto) {
    hipLaunchKernelGGL(k_tile_gather<c()>, flat_grid((size_t)n * th * tw), dim3(256), 0, (hipStream_t)stream, pic,
                       Strides4{0, c_stride, row_stride, px_stride}, H, W, reinterpret_cast<const TileAxis*>(table), nty, ntx, th,
                       tw, t0, n, out);
  });
  return check_launch("tile_gather");
}

// checks and launches the stitch for one destination
static int stitch(const char* what, const float* tiles, const Strides4& s, int C, int oth, int otw, const int32_t* table, int nty,
                  int ntx, int t0, int n, int kind, const PicDst& dst, int OH, int OW, void* stream) {
  int rc = stitch_args_ok(what, tiles, s, C, oth, otw, table, nty, ntx, t0, n, kind == kDstF32 ? (const void*)dst.f32 : dst.u8, OH,
                          OW);
  if (rc == SRK_OK) rc = pic_dst_ok(what, C, dst.cb, dst.cr);
  if (rc != SRK_OK) return rc;
  launch_pic(C, kind, [&](auto c, auto d) {
    hipLaunchKernelGGL((k_tile_stitch<c(), d()>), stitch_grid(oth, OH, OW, ntx, t0, n), dim3(256), 0, (hipStream_t)stream, tiles, s,
                       oth, otw, reinterpret_cast<const TileAxis*>(table), nty, ntx, t0, n, dst, OH, OW);
  });
  return check_launch(what);
}

extern "C" int srk_tile_stitch_f32(const float* tiles, int64_t n_stride, int64_t c_stride, int64_t row_stride, int64_t px_stride,
                                   int C, int oth, int otw, const int32_t* table, int nty, int ntx, int t0, int n, float* out,
                                   int OH, int OW, void* stream) {
  return stitch("tile_stitch_f32", tiles, {n_stride, c_stride, row_stride, px_stride}, C, oth, otw, table, nty, ntx, t0, n, kDstF32,
                {out, nullptr, nullptr, nullptr}, OH, OW, stream);
}

extern "C" int srk_tile_stitch_u8(const float* tiles, int64_t n_stride, int64_t c_stride, int64_t row_stride, int64_t px_stride,
                                  int C, int oth, int otw, const int32_t* table, int nty, int ntx, int t0, int n,
                                  const uint8_t* cb, const uint8_t* cr, uint8_t* out, int OH, int OW, void* stream) {
  return stitch("tile_stitch_u8", tiles, {n_stride, c_stride, row_stride, px_stride}, C, oth, otw, table, nty, ntx, t0, n,
                cb ? kDstYcc : kDstU8, {nullptr, out, cb, cr}, OH, OW, stream);
}
