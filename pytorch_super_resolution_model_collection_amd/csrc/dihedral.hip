// Geometric self-ensemble (x8, the "+" of EDSR+): the eight flips / rotations of a batch of pictures in ONE launch
// (k_dihedral_variants) and, after the net, the inverse transforms and the ordered mean of the eight results in ONE launch
// (k_dihedral_merge) -- as the fp32 picture, or straight as the final interleaved 8-bit picture (quantised like k_to_u8,
// or quantised and converted with 8-bit chroma planes like k_ycc_to_rgb: the fp32 mean is then never written).
//
// Numbering (sr_trainers.py): k = 4 m + r, T_k(x) = rot90(flip_W(x) if m else x, r).  A source pixel (a, b)
// of an H x W picture lands in variant k at
//     k = 0 (a, b)           k = 2 (H-1-a, W-1-b)    k = 4 (a, W-1-b)      k = 6 (H-1-a, b)           H x W, the "even" group
//     k = 1 (W-1-b, a)       k = 3 (b, H-1-a)        k = 5 (b, a)          k = 7 (W-1-b, H-1-a)       W x H, the "odd" group
// i.e. every variant is (transpose?, flip a?, flip b?), all eight combinations once.  Slot v = 4 * odd + j of the output
// allocation holds k = 2 j + odd; with fa = v & 1 and fb = bit v of 0x96 the landing place is (a', b') = (fa ? H-1-a : a,
// fb ? W-1-b : b), transposed for the odd group.  The merge reads the same places: E(a, b) = 0.125 * sum_k y_k(place_k(a, b)),
// summed in fp32 in the order k = 0 .. 7.
//
// Access pattern.  Half of all traffic is transposed, so everything goes through an LDS tile of 32 x 32 pixels per channel,
// rows padded to 33 floats (channel planes a multiple of 32 floats apart, so the bank of (c, a, b) is (a + b) mod 32).
// Global memory is only ever touched along contiguous LINES (a stretch of one row of one image: 32 C floats of a
// channels-last image, 32 floats of a planar one, 32 OC bytes of the 8-bit picture).  One half-wave (32 lanes: the lane
// group of ds_read_b32 / ds_write_b32) owns a line, and lane q owns the q-th 16-byte-ALIGNED chunk of memory the line
// touches: a whole chunk inside the line is one 16-byte access, the clipped first and last chunks are scalar, so every
// byte is read / written exactly once whatever the width, with no atomics.  The lanes of a half-wave then touch LDS at
// distinct pixels of ONE tile row (row-wise access: banks a + b, b distinct) or of ONE tile column (the transposed
// access: banks a + b, a distinct): neither side is bank-conflicted, and neither side of a transposed copy walks memory
// with a stride of the width.  The price is idle lanes where a line has fewer than 32 chunks (9 for one channel; the
// one-channel 8-bit modes keep that layout and pack four lanes' bytes into one store, see k_dihedral_merge).
#include "color_common.h"

namespace srk {

constexpr int kDT = 32;                 // tile side in pixels
constexpr int kDLd = kDT + 1;           // padded LDS row
constexpr int kDPlane = kDT * kDLd;     // one channel (a multiple of 32 floats)
constexpr int kVarHalves = 8;           // half-waves of a block of k_dihedral_variants (256 threads)
constexpr int kMergeHalves = 16;        // ... of k_dihedral_merge (512: half the running sums per lane)

__device__ __forceinline__ int flip_a(int v) { return v & 1; }
__device__ __forceinline__ int flip_b(int v) { return (0x96 >> v) & 1; }

// rows [i0, i0 + th) x columns [j0, j0 + tw) of one image (element strides sc, sh, sw) -> lds[c][row][col].  Lines are the
// tile rows of a channels-last image (tw C contiguous floats) or the rows of each channel plane otherwise.
template <int C, int HALVES>
__device__ __forceinline__ void load_tile(const float* __restrict__ img, long long sc, long long sh, long long sw, int i0, int j0,
                                          int th, int tw, float* lds) {
  const int half = threadIdx.x >> 5, lane = threadIdx.x & 31;
  const bool cl = C > 1 && sc == 1 && sw == C;
  const int nlines = cl ? th : C * th;
  const int L = cl ? tw * C : tw;
  const long long step = cl ? 1 : sw;
  for (int ln = half; ln < nlines; ln += HALVES) {
    const int c0 = cl ? 0 : ln / th, a = cl ? ln : ln - c0 * th;
    const float* p = img + c0 * sc + (long long)(i0 + a) * sh + (long long)j0 * sw;
    const int d = step == 1 ? (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3) : 0;   // floats past a 16-byte boundary
    for (int q = lane; 4 * q < L + d; q += 32) {
      const int lo = 4 * q - d;
      float v[4];
      if (step == 1 && lo >= 0 && lo + 4 <= L) {
        const float4 f = *reinterpret_cast<const float4*>(p + lo);
        v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (lo + u >= 0 && lo + u < L) ? p[(lo + u) * step] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = lo + u;
        if (i >= 0 && i < L) {
          const int c = cl ? i % C : c0, b = cl ? i / C : i;
          lds[c * kDPlane + a * kDLd + b] = v[u];
        }
      }
    }
  }
}

// x [N][C][H][W] through element strides -> out: 4 N channels-last images of H x W (slots v = 0 .. 3 of image n at
// 4 n + v), then 4 N channels-last images of W x H (v = 4 .. 7 at 4 n + v - 4).  One block per 32 x 32 source tile: the
// tile is read once and written eight times.
template <int C>
__global__ __launch_bounds__(256) void k_dihedral_variants(const float* __restrict__ x, long long sn, long long sc, long long sh,
                                                           long long sw, int N, int H, int W, int tiles_y, int tiles_x,
                                                           float* __restrict__ out) {
  __shared__ float lds[C * kDPlane];
  const int half = threadIdx.x >> 5, lane = threadIdx.x & 31;
  const int tile = blockIdx.x % (tiles_y * tiles_x), n = blockIdx.x / (tiles_y * tiles_x);
  const int a0 = tile / tiles_x * kDT, b0 = tile % tiles_x * kDT;
  const int th = H - a0 < kDT ? H - a0 : kDT, tw = W - b0 < kDT ? W - b0 : kDT;
  load_tile<C, kVarHalves>(x + n * sn, sc, sh, sw, a0, b0, th, tw, lds);
  __syncthreads();
  const size_t image = (size_t)H * W * C;
  for (int item = half; item < 8 * kDT; item += kVarHalves) {
    const int v = item >> 5, line = item & 31;
    const bool tr = v >= 4;
    const int fa = flip_a(v), fb = flip_b(v);
    const int nlines = tr ? tw : th;       // destination rows of this tile
    if (line >= nlines) continue;
    const int npx = tr ? th : tw;          // destination pixels per row
    // the source row (tr: column) this destination row is, and where the row lands
    const int Wd = tr ? H : W;
    const int drow = tr ? (fb ? W - 1 - (b0 + line) : b0 + line) : (fa ? H - 1 - (a0 + line) : a0 + line);
    const int dcol = tr ? (fa ? H - a0 - th : a0) : (fb ? W - b0 - tw : b0);
    const bool rev = tr ? fa : fb;         // the destination row runs against the source
    float* d = out + ((size_t)(tr ? 4 : 0) * N + (size_t)4 * n + (v & 3)) * image + ((size_t)drow * Wd + dcol) * C;
    const int L = npx * C;
    const int dl = (int)((reinterpret_cast<uintptr_t>(d) >> 2) & 3);
    const int q = lane;
    if (4 * q >= L + dl) continue;
    const int lo = 4 * q - dl;
    float val[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = lo + u;
      if (e >= 0 && e < L) {
        const int pj = e / C, c = e - pj * C;
        const int s = rev ? npx - 1 - pj : pj;
        val[u] = tr ? lds[c * kDPlane + s * kDLd + line] : lds[c * kDPlane + line * kDLd + s];
      } else {
        val[u] = 0.f;
      }
    }
    if (lo >= 0 && lo + 4 <= L) {
      *reinterpret_cast<float4*>(d + lo) = make_float4(val[0], val[1], val[2], val[3]);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (lo + u >= 0 && lo + u < L) d[lo + u] = val[u];
    }
  }
}

// even [4N][C][oh][ow], odd [4N][C][ow][oh] through element strides -> E.  One block per 32 x 32 tile of E: the eight
// input tiles pass through the LDS tile one after another (k = 0 .. 7, the order of the sum) while every lane keeps the
// running sums of the destination chunks it owns in registers.  DST: kDstF32 is [N][C][oh][ow]; the 8-bit kinds are one
// picture (N = 1).
template <int C, int DST>
__global__ __launch_bounds__(512) void k_dihedral_merge(const float* __restrict__ even, Strides4 se, const float* __restrict__ odd,
                                                        Strides4 so, int oh, int ow, int tiles_y, int tiles_x, PicDst dst) {
  // One-channel 8-bit destinations (U8 with C = 1, YCC) use the lane layout of the fp32 merge, 4 pixels per lane, and four
  // neighbouring lanes (a GROUP: one 16-byte-aligned chunk of 16 pixels) bring their bytes together with cross-lane moves
  // before the 16-byte stores: as many lanes at work as in the fp32 merge, the same conflict-free LDS reads.
  constexpr bool PACK = DST != kDstF32 && C == 1;
  constexpr int NV = DST == kDstF32 || PACK ? 4 : 16;              // values a lane owns per item
  constexpr int ITEMS = (DST == kDstF32 ? C : 1) * kDT / kMergeHalves;   // destination lines per half-wave
  __shared__ float lds[C * kDPlane];
  __shared__ alignas(16) int16_t ctab[DST == kDstYcc ? kInvTabs * 256 : 8];
  if (DST == kDstYcc) stage_tables<kInvTabs, 32 * kMergeHalves>(kColorDev.inv, ctab);
  const int half = threadIdx.x >> 5, lane = threadIdx.x & 31;
  const int tile = blockIdx.x % (tiles_y * tiles_x), n = blockIdx.x / (tiles_y * tiles_x);
  const int a0 = tile / tiles_x * kDT, b0 = tile % tiles_x * kDT;
  const int th = oh - a0 < kDT ? oh - a0 : kDT, tw = ow - b0 < kDT ? ow - b0 : kDT;

  // the destination line of item `it` (F32: row `la` of channel `ch`; 8-bit: row `la`), its length L in destination
  // elements (floats, bytes, or pixels for YCC) and the first element `lo` of this lane's share of it (may be < 0): lanes
  // are laid out from the 16-byte boundary at or before the line's first byte in the destination
  auto item_of = [&](int it, int& ch, int& la, int& L, int& lo) -> bool {
    const int line = half + kMergeHalves * it;
    int d;
    if (DST == kDstF32) {
      ch = line / kDT, la = line - ch * kDT;
      L = tw;
      const float* p = dst.f32 + (((size_t)n * C + ch) * oh + a0 + la) * ow + b0;
      d = (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3);
    } else {
      ch = 0, la = line;
      const size_t px = (size_t)(a0 + la) * ow + b0;
      if (DST == kDstU8) {
        L = tw * C;
        d = (int)(reinterpret_cast<uintptr_t>(dst.u8 + px * C) & 15);
      } else {
        L = tw;
        // pixels past the pixel whose 3 bytes start a 16-byte chunk of the picture: 3 (px - d) + out = 0 (mod 16), and
        // 11 is the inverse of 3 mod 16
        d = (int)((px + 11 * reinterpret_cast<uintptr_t>(dst.u8)) & 15);
      }
    }
    lo = NV * lane - d;
    return la < th && NV * lane < L + d;
  };

  float acc[ITEMS][NV];
  if (PACK) {
#pragma unroll
    for (int it = 0; it < ITEMS; ++it)
#pragma unroll
      for (int u = 0; u < NV; ++u) acc[it][u] = 0.f;
  }
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    const int v = (k & 1) * 4 + (k >> 1);
    const bool tr = k & 1;
    const int fa = flip_a(v), fb = flip_b(v);
    const float* img = tr ? odd + ((long long)4 * n + (v & 3)) * so.n : even + ((long long)4 * n + v) * se.n;
    const Strides4 s = tr ? so : se;
    if (k) __syncthreads();   // the previous variant's tile has been consumed
    if (tr)
      load_tile<C, kMergeHalves>(img, s.c, s.h, s.w, fb ? ow - b0 - tw : b0, fa ? oh - a0 - th : a0, tw, th, lds);
    else
      load_tile<C, kMergeHalves>(img, s.c, s.h, s.w, fa ? oh - a0 - th : a0, fb ? ow - b0 - tw : b0, th, tw, lds);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      int ch, la, L, lo;
      if (!item_of(it, ch, la, L, lo)) continue;
      const int sa = fa ? th - 1 - la : la;
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int e = lo + u;
        float y = 0.f;
        if (e >= 0 && e < L) {
          const int lb = DST == kDstU8 ? e / C : e;
          const int c = DST == kDstU8 ? e - lb * C : ch;
          const int sb = fb ? tw - 1 - lb : lb;
          y = tr ? lds[c * kDPlane + sb * kDLd + sa] : lds[c * kDPlane + sa * kDLd + sb];
        }
        acc[it][u] = k ? acc[it][u] + y : y;
      }
    }
  }

  if constexpr (PACK) {
    // every lane runs the cross-lane moves (no early exit before them); `whole` is the same in the four lanes of a group
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      int ch, la, L, lo;
      const bool ok = item_of(it, ch, la, L, lo);
      const int sub = lane & 3, g0 = lo - 4 * sub;            // the group's first pixel of the line
      const bool whole = la < th && g0 >= 0 && g0 + 16 <= L;
      const long long row = (long long)(a0 + la) * ow + b0;   // the line's first pixel in the picture
      unsigned yq[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) yq[u] = quant_u8(acc[it][u] * 0.125f);
      if (DST == kDstU8) {
        const unsigned w = yq[0] | yq[1] << 8 | yq[2] << 16 | yq[3] << 24;
        const unsigned n1 = __shfl_down(w, 1), n2 = __shfl_down(w, 2), n3 = __shfl_down(w, 3);
        if (whole) {
          if (sub == 0) *reinterpret_cast<uint4*>(dst.u8 + row + g0) = make_uint4(w, n1, n2, n3);
        } else if (ok) {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (lo + u >= 0 && lo + u < L) dst.u8[row + lo + u] = (unsigned char)yq[u];
        }
      } else {
        // this lane's 4 bytes of each chroma plane: its word of the group's 16-byte chunk where that is aligned (the four
        // lanes of a group read the same 16 bytes), else byte by byte
        unsigned cw[2] = {0, 0};
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
          const unsigned char* plane = pl ? dst.cr : dst.cb;
          if (whole && aligned16(plane + row + g0)) {
            const uint4 q = *reinterpret_cast<const uint4*>(plane + row + g0);
            cw[pl] = sub == 0 ? q.x : (sub == 1 ? q.y : (sub == 2 ? q.z : q.w));
          } else if (ok) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (lo + u >= 0 && lo + u < L) cw[pl] |= (unsigned)plane[row + lo + u] << (u * 8);
          }
        }
        unsigned t[3] = {0, 0, 0};   // this lane's 12 bytes of the picture
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          int rr, gg, bb;
          ycc_to_rgb_px(ctab, (int)yq[u], (int)((cw[0] >> (u * 8)) & 255u), (int)((cw[1] >> (u * 8)) & 255u), rr, gg, bb);
          put_rgb(t, u, rr, gg, bb);
        }
        // the group's 48 bytes are words 3 sub .. 3 sub + 2 of lanes sub = 0 .. 3; lane sub < 3 stores words 4 sub .. 4 sub + 3
        const unsigned n0 = __shfl_down(t[0], 1), n1 = __shfl_down(t[1], 1), n2 = __shfl_down(t[2], 1);
        if (whole) {
          unsigned char* d = dst.u8 + 3 * (row + g0) + 16 * sub;
          if (sub == 0) *reinterpret_cast<uint4*>(d) = make_uint4(t[0], t[1], t[2], n0);
          if (sub == 1) *reinterpret_cast<uint4*>(d) = make_uint4(t[1], t[2], n0, n1);
          if (sub == 2) *reinterpret_cast<uint4*>(d) = make_uint4(t[2], n0, n1, n2);
        } else if (ok) {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (lo + u >= 0 && lo + u < L) {
#pragma unroll
              for (int c = 0; c < 3; ++c) dst.u8[3 * (row + lo + u) + c] = (unsigned char)get_byte(t, 3 * u + c);
            }
        }
      }
    }
  } else {
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      int ch, la, L, lo;
      if (!item_of(it, ch, la, L, lo)) continue;
      const bool whole = lo >= 0 && lo + NV <= L;
      if (DST == kDstF32) {
        float* d = dst.f32 + (((size_t)n * C + ch) * oh + a0 + la) * ow + b0 + lo;
        if (whole) {
          *reinterpret_cast<float4*>(d) = make_float4(acc[it][0] * 0.125f, acc[it][1] * 0.125f, acc[it][2] * 0.125f, acc[it][3] * 0.125f);
        } else {
#pragma unroll
          for (int u = 0; u < NV; ++u)
            if (lo + u >= 0 && lo + u < L) d[u] = acc[it][u] * 0.125f;
        }
      } else {   // interleaved 8-bit RGB: a lane owns one 16-byte chunk
        unsigned char* d = dst.u8 + ((size_t)(a0 + la) * ow + b0) * C + lo;
        unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < NV; ++u) w[u >> 2] |= quant_u8(acc[it][u] * 0.125f) << ((u & 3) * 8);
        if (whole) {
          *reinterpret_cast<uint4*>(d) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
          for (int u = 0; u < NV; ++u)
            if (lo + u >= 0 && lo + u < L) d[u] = (unsigned char)get_byte(w, u);
        }
      }
    }
  }
}

static int dihedral_grid(const char* what, int N, int H, int W, int& tiles_y, int& tiles_x, dim3& grid) {
  tiles_y = (H + kDT - 1) / kDT, tiles_x = (W + kDT - 1) / kDT;
  const long long blocks = (long long)N * tiles_y * tiles_x;
  SRK_REQUIRE(blocks <= 0x7fffffffLL, "%s: %d images of %d x %d are more tiles than a grid holds", what, N, H, W);
  grid = dim3((unsigned)blocks);
  return SRK_OK;
}

static int merge_args_ok(const char* what, const void* even, const Strides4& se, const void* odd, const Strides4& so, int N,
                         int C, int oh, int ow, const void* out) {
  SRK_REQUIRE(even && odd && out, "%s: null pointer", what);
  SRK_REQUIRE(C == 1 || C == 3, "%s: C must be 1 or 3 (got %d)", what, C);
  SRK_REQUIRE(N > 0 && oh > 0 && ow > 0, "%s: non-positive dims (%d images of %d x %d)", what, N, oh, ow);
  SRK_REQUIRE(se.n >= 0 && se.c >= 0 && se.h >= 0 && se.w >= 0 && so.n >= 0 && so.c >= 0 && so.h >= 0 && so.w >= 0,
              "%s: negative strides", what);
  return SRK_OK;
}

}  // namespace srk

using namespace srk;

extern "C" int srk_dihedral_variants(const float* x, int64_t n_stride, int64_t c_stride, int64_t row_stride, int64_t px_stride,
                                     int N, int C, int H, int W, float* out, void* stream) {
  SRK_REQUIRE(x && out, "dihedral_variants: null pointer");
  SRK_REQUIRE(C == 1 || C == 3, "dihedral_variants: C must be 1 or 3 (got %d)", C);
  SRK_REQUIRE(N > 0 && H > 0 && W > 0, "dihedral_variants: non-positive dims (%d images of %d x %d)", N, H, W);
  SRK_REQUIRE(n_stride >= 0 && c_stride >= 0 && row_stride >= 0 && px_stride >= 0, "dihedral_variants: negative strides");
  int ty, tx;
  dim3 grid;
  const int rc = dihedral_grid("dihedral_variants", N, H, W, ty, tx, grid);
  if (rc != SRK_OK) return rc;
  launch_pic(C, kDstF32, [&](auto c, auto) {
    hipLaunchKernelGGL(k_dihedral_variants<c()>, grid, dim3(256), 0, (hipStream_t)stream, x, (long long)n_stride,
                       (long long)c_stride, (long long)row_stride, (long long)px_stride, N, H, W, ty, tx, out);
  });
  return check_launch("dihedral_variants");
}

// checks and launches the merge for one destination
static int merge(const char* what, const float* even, const int64_t* even_strides, const float* odd, const int64_t* odd_strides,
                 int N, int C, int oh, int ow, int kind, const PicDst& dst, void* stream) {
  SRK_REQUIRE(even_strides && odd_strides, "%s: null pointer", what);
  const Strides4 se = strides4(even_strides), so = strides4(odd_strides);
  int rc = merge_args_ok(what, even, se, odd, so, N, C, oh, ow, kind == kDstF32 ? (const void*)dst.f32 : dst.u8);
  if (rc == SRK_OK) rc = pic_dst_ok(what, C, dst.cb, dst.cr);
  int ty, tx;
  dim3 grid;
  if (rc == SRK_OK) rc = dihedral_grid(what, N, oh, ow, ty, tx, grid);
  if (rc != SRK_OK) return rc;
  launch_pic(C, kind, [&](auto c, auto d) {
    hipLaunchKernelGGL((k_dihedral_merge<c(), d()>), grid, dim3(32 * kMergeHalves), 0, (hipStream_t)stream, even, se, odd, so, oh,
                       ow, ty, tx, dst);
  });
  return check_launch(what);
}

extern "C" int srk_dihedral_merge_f32(const float* even, const int64_t* even_strides, const float* odd, const int64_t* odd_strides,
                                      int N, int C, int oh, int ow, float* out, void* stream) {
  return merge("dihedral_merge_f32", even, even_strides, odd, odd_strides, N, C, oh, ow, kDstF32, {out, nullptr, nullptr, nullptr},
               stream);
}

extern "C" int srk_dihedral_merge_u8(const float* even, const int64_t* even_strides, const float* odd, const int64_t* odd_strides,
                                     int C, int oh, int ow, const uint8_t* cb, const uint8_t* cr, uint8_t* out, void* stream) {
  return merge("dihedral_merge_u8", even, even_strides, odd, odd_strides, 1, C, oh, ow, cb ? kDstYcc : kDstU8,
               {nullptr, out, cb, cr}, stream);
}
