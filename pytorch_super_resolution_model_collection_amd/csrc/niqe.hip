// NIQE's natural-scene-statistics features (Mittal, Soundararajan, Bovik 2013, as BasicSR's calculate_niqe states them) of
// one picture on the device: [blocks, 36] doubles, 18 per scale.  include/srk.h has the definition, DESIGN.md 34 the rest.
//
// k_niqe_scale<S>: a workgroup owns one block of the grid at scale S.  It stages the block and its 3-pixel halo into LDS
// -- scale 1 from the picture through its element strides, quantised, turned to luma and cropped on the way (bytes 16 ..
// 235: exact in fp32); scale 2 from the fp64 plane P_2 -- with the plane's borders replicated.  Scale 1 then writes its
// quarter of P_2 from the staged luma (the 2:1 shrink reads 2i - 3 .. 2i + 4: the very halo the window needs, and its
// reflections land inside the block).  The separable 7 x 7 window runs through a strip buffer of kNiqeStrip + 6 rows; the
// MSCN values of the whole block stay in LDS, so the four circular neighbour products are LDS reads.  Each thread adds its
// values of the five maps into 30 sums in index order, a wave adds its lanes by butterfly, thread `map` adds the 8 wave
// partials in wave order and fits its map.  No atomics: two calls give the same bits.  Neither the luma plane of scale 1
// nor any MSCN map goes to memory.
#include <type_traits>
#include <vector>

#include "niqe_common.h"

namespace srk {

// 8 waves, 2 a SIMD: the phases are latency-bound, and 16 waves would cap a thread at 128 VGPRs, under what the 31 fp64
// sums need beside the address arithmetic (164 bytes of scratch a lane)
constexpr int kNiqeThreads = 512, kNiqeWaves = kNiqeThreads / kWave;
constexpr int kNiqeStrip = 15;                               // output rows of one pass of the window (21 x 96 = 4 x 512 - 32)
constexpr int kNiqeVals = kNiqeMaps * kNiqeSums + 1;         // a thread's sums: 5 maps x 6, then sigma
constexpr int kNiqePartStride = 32;

struct NiqeJob {
  NiqeSrc src;
  int Hc, Wc;   // the crop at scale 1
  int nw;       // blocks along a row of the grid
  int b;        // block side at this scale
  const double* tables;
  double* p2;   // [Hc / 2][Wc / 2]
  double* features;
  double* sharpness;
};

template <int S>
static size_t niqe_lds_bytes(int b) {
  const size_t tb = b + kNiqeHalo;
  return ((size_t)b * b + (size_t)2 * (kNiqeStrip + kNiqeHalo) * b + kNiqeWaves * kNiqePartStride) * sizeof(double) +
         tb * tb * (S == 1 ? sizeof(float) : sizeof(double));
}

// one value's per-wave partials added in wave order
__device__ __forceinline__ double niqe_sum_waves(const double* part) {
  double t = part[0];
  for (int w = 1; w < kNiqeWaves; ++w) t += part[w * kNiqePartStride];
  return t;
}

template <int S>
__global__ __launch_bounds__(kNiqeThreads) void k_niqe_scale(NiqeJob job) {
  using T = std::conditional_t<S == 1, float, double>;
  extern __shared__ __align__(16) unsigned char niqe_lds[];
  const int b = job.b, tb = b + kNiqeHalo, hplane = (kNiqeStrip + kNiqeHalo) * b;
  double* nt = reinterpret_cast<double*>(niqe_lds);       // [b][b]       the block's MSCN values
  double* hs = nt + b * b;                                // [2][strip + 6][b]  row sums of P and P^2
  double* part = hs + 2 * hplane;                         // [waves][32]  per-wave partials
  T* tile = reinterpret_cast<T*>(part + kNiqeWaves * kNiqePartStride);   // [tb][tb]  the staged plane
  const int tid = threadIdx.x;
  const int by = blockIdx.x / job.nw, bx = blockIdx.x - by * job.nw;
  const int PH = S == 1 ? job.Hc : job.Hc / 2, PW = S == 1 ? job.Wc : job.Wc / 2;
  const int y0 = by * b - kNiqeR, x0 = bx * b - kNiqeR;

  for (int i = tid; i < tb * tb; i += kNiqeThreads) {
    const int r = i / tb, c = i - r * tb;
    const int y = min(max(y0 + r, 0), PH - 1), x = min(max(x0 + c, 0), PW - 1);
    if constexpr (S == 1)
      tile[i] = (float)niqe_src_luma(job.src, y, x);
    else
      tile[i] = job.p2[(int64_t)y * PW + x];
  }
  __syncthreads();

  if constexpr (S == 1) {   // this block's (b/2) x (b/2) values of P_2
    const int half = b >> 1, W2 = job.Wc >> 1;
    for (int i = tid; i < half * half; i += kNiqeThreads) {
      const int r = i / half, c = i - r * half;
      const int oi = by * half + r, oj = bx * half + c;
      int lx[kNiqeShrinkTaps];
#pragma unroll
      for (int k = 0; k < kNiqeShrinkTaps; ++k) lx[k] = niqe_reflect(2 * oj - 3 + k, job.Wc) - x0;
      double acc = 0.0;
#pragma unroll
      for (int ky = 0; ky < kNiqeShrinkTaps; ++ky) {
        const float* row = tile + (niqe_reflect(2 * oi - 3 + ky, job.Hc) - y0) * tb;
        double h = 0.0;
#pragma unroll
        for (int kx = 0; kx < kNiqeShrinkTaps; ++kx) h += niqe_shrink_weight(kx) * (double)row[lx[kx]];
        acc += niqe_shrink_weight(ky) * h;
      }
      job.p2[(int64_t)oi * W2 + oj] = acc;
    }
  }

  double val[kNiqeVals];
#pragma unroll
  for (int q = 0; q < kNiqeVals; ++q) val[q] = 0.0;

  for (int r0 = 0; r0 < b; r0 += kNiqeStrip) {
    const int rows = min(kNiqeStrip, b - r0);
    for (int i = tid; i < (rows + kNiqeHalo) * b; i += kNiqeThreads) {   // horizontal: lanes along a row
      const int r = i / b, c = i - r * b;
      const T* p = tile + (r0 + r) * tb + c;
      double m = 0.0, q = 0.0;
#pragma unroll
      for (int k = 0; k < kNiqeTaps; ++k) {
        const double v = (double)p[k], g = kNiqeWinDev.g[k];
        m = fma(g, v, m), q = fma(g, v * v, q);
      }
      hs[i] = m, hs[hplane + i] = q;
    }
    __syncthreads();
    for (int i = tid; i < rows * b; i += kNiqeThreads) {                 // vertical, then the normalisation
      const int r = i / b, c = i - r * b;
      double mu = 0.0, e2 = 0.0;
#pragma unroll
      for (int k = 0; k < kNiqeTaps; ++k) {
        const double g = kNiqeWinDev.g[k];
        mu = fma(g, hs[i + k * b], mu), e2 = fma(g, hs[hplane + i + k * b], e2);
      }
      const double p = (double)tile[(r0 + r + kNiqeR) * tb + c + kNiqeR];
      nt[r0 * b + i] = niqe_mscn(p, mu, e2);
      if constexpr (S == 1) val[kNiqeVals - 1] += niqe_sigma(mu, e2);
    }
    __syncthreads();   // hs is written again; after the last strip nt is complete
  }

  for (int i = tid; i < b * b; i += kNiqeThreads) {
    const int r = i / b, c = i - r * b;
    const double v = nt[i];
    niqe_accumulate(val, v);
#pragma unroll
    for (int k = 1; k < kNiqeMaps; ++k) {
      int rr, cc;
      niqe_roll_source(k, r, c, b, rr, cc);
      niqe_accumulate(val + k * kNiqeSums, v * nt[rr * b + cc]);
    }
  }

  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int q = 0; q < kNiqeVals; ++q) {
    const double t = wave_sum_d(val[q]);
    if (lane == 0) part[wv * kNiqePartStride + q] = t;
  }
  __syncthreads();
  const double M = (double)b * (double)b;
  if (tid < kNiqeMaps) {
    double s[kNiqeSums];
    for (int j = 0; j < kNiqeSums; ++j) s[j] = niqe_sum_waves(part + tid * kNiqeSums + j);
    niqe_fit(s, M, job.tables, tid,
             job.features + (int64_t)blockIdx.x * SRK_NIQE_FEATURES + (S - 1) * (SRK_NIQE_FEATURES / 2) +
                 niqe_feature_offset(tid));
  }
  if (S == 1 && tid == kNiqeMaps && job.sharpness) {
    job.sharpness[blockIdx.x] = niqe_sum_waves(part + kNiqeVals - 1) / M;
  }
}

// the argument rules the device call and the host twin share; on success the crop and the grid
static int niqe_check(const void* img, const void* tables, const void* features, int C, int H, int W, int shave, int block,
                      const char* who, int& nh, int& nw) {
  SRK_REQUIRE(img && tables && features, "%s: null pointer (img %p, tables %p, features %p)", who, img, tables, features);
  SRK_REQUIRE(C == 1 || C == 3, "%s: takes 1 or 3 channels (got %d)", who, C);
  SRK_REQUIRE(H > 0 && W > 0, "%s: bad dims (%d x %d)", who, H, W);
  SRK_REQUIRE(shave >= 0, "%s: negative shave (%d)", who, shave);
  SRK_REQUIRE(block >= kNiqeMinBlock && block <= kNiqeMaxBlock && block % 2 == 0,
              "%s: block must be even and in %d .. %d (got %d)", who, kNiqeMinBlock, kNiqeMaxBlock, block);
  const int64_t h = (int64_t)H - 2 * (int64_t)shave, w = (int64_t)W - 2 * (int64_t)shave;
  nh = h > 0 ? (int)(h / block) : 0, nw = w > 0 ? (int)(w / block) : 0;
  SRK_REQUIRE((int64_t)nh * nw >= 2,
              "%s: a picture of %d x %d with %d pixels shaved from each side holds %d x %d blocks of %d x %d, fewer than 2",
              who, H, W, shave, nh, nw, block, block);
  return SRK_OK;
}

static NiqeSrc niqe_src(const void* img, int is_u8, const int64_t* strides, int C, int H, int W, int shave) {
  NiqeSrc s;
  s.img = img, s.is_u8 = is_u8, s.C = C;
  if (strides)
    s.sc = strides[0], s.sh = strides[1], s.sw = strides[2];
  else
    s.sc = (int64_t)H * W, s.sh = W, s.sw = 1;   // NULL: dense [C][H][W]
  s.origin = shave * (s.sh + s.sw);
  return s;
}

// One scale on the host: window with replicated borders over the whole plane, then every block's sums in row-major
// order and the fit.
static void niqe_host_scale(const std::vector<double>& P, int PH, int PW, int b, const double* tables, double* features,
                            double* sharpness) {
  const double* g = kNiqeWinHost.g;
  std::vector<double> hm((size_t)PH * PW), hq((size_t)PH * PW), n((size_t)PH * PW), sg((size_t)PH * PW);
  for (int y = 0; y < PH; ++y)
    for (int x = 0; x < PW; ++x) {
      double m = 0.0, q = 0.0;
      for (int k = 0; k < kNiqeTaps; ++k) {
        const int xx = x + k - kNiqeR < 0 ? 0 : (x + k - kNiqeR >= PW ? PW - 1 : x + k - kNiqeR);
        const double v = P[(size_t)y * PW + xx];
        m = fma(g[k], v, m), q = fma(g[k], v * v, q);
      }
      hm[(size_t)y * PW + x] = m, hq[(size_t)y * PW + x] = q;
    }
  for (int y = 0; y < PH; ++y)
    for (int x = 0; x < PW; ++x) {
      double mu = 0.0, e2 = 0.0;
      for (int k = 0; k < kNiqeTaps; ++k) {
        const int yy = y + k - kNiqeR < 0 ? 0 : (y + k - kNiqeR >= PH ? PH - 1 : y + k - kNiqeR);
        mu = fma(g[k], hm[(size_t)yy * PW + x], mu), e2 = fma(g[k], hq[(size_t)yy * PW + x], e2);
      }
      n[(size_t)y * PW + x] = niqe_mscn(P[(size_t)y * PW + x], mu, e2);
      sg[(size_t)y * PW + x] = niqe_sigma(mu, e2);
    }
  const int nh = PH / b, nw = PW / b;
  const double M = (double)b * (double)b;
  for (int by = 0; by < nh; ++by)
    for (int bx = 0; bx < nw; ++bx) {
      double s[kNiqeMaps][kNiqeSums] = {}, ssum = 0.0;
      const double* B = n.data() + (size_t)by * b * PW + (size_t)bx * b;
      for (int r = 0; r < b; ++r)
        for (int c = 0; c < b; ++c) {
          const double v = B[(size_t)r * PW + c];
          niqe_accumulate(s[0], v);
          for (int k = 1; k < kNiqeMaps; ++k) {
            int rr, cc;
            niqe_roll_source(k, r, c, b, rr, cc);
            niqe_accumulate(s[k], v * B[(size_t)rr * PW + cc]);
          }
          ssum += sg[((size_t)by * b + r) * PW + (size_t)bx * b + c];
        }
      double* f = features + ((size_t)by * nw + bx) * SRK_NIQE_FEATURES;
      for (int k = 0; k < kNiqeMaps; ++k) niqe_fit(s[k], M, tables, k, f + niqe_feature_offset(k));
      if (sharpness) sharpness[(size_t)by * nw + bx] = ssum / M;
    }
}

}  // namespace srk

using namespace srk;

extern "C" int srk_niqe_tables_host(double* out) {
  SRK_REQUIRE(out, "niqe_tables_host: null pointer");
  for (int j = 0; j < kNiqeTable; ++j) {
    const double g = niqe_gam(j);
    const double g1 = tgamma(1.0 / g), g2 = tgamma(2.0 / g), g3 = tgamma(3.0 / g);
    out[j] = g2 * g2 / (g1 * g3);
    out[kNiqeTable + j] = sqrt(g1 / g3);
    out[2 * kNiqeTable + j] = g2 / g1;
  }
  return SRK_OK;
}

extern "C" size_t srk_niqe_workspace_bytes(int H, int W, int block) {
  if (H <= 0 || W <= 0 || block < kNiqeMinBlock || block > kNiqeMaxBlock || block % 2) return 0;
  const size_t half = block / 2;
  return (size_t)(H / block) * (size_t)(W / block) * half * half * sizeof(double);   // P_2 with no shave: the largest
}

extern "C" int srk_niqe_features(const void* img, int is_u8, const int64_t* strides, int C, int H, int W, int shave,
                                 int block, const double* tables, double* features, double* sharpness, void* workspace,
                                 void* stream) {
  int nh, nw;
  if (int rc = niqe_check(img, tables, features, C, H, W, shave, block, "niqe_features", nh, nw)) return rc;
  SRK_REQUIRE(workspace, "niqe_features: null workspace");
  NiqeJob job;
  job.src = niqe_src(img, is_u8, strides, C, H, W, shave);
  job.Hc = nh * block, job.Wc = nw * block, job.nw = nw;
  job.tables = tables, job.p2 = (double*)workspace, job.features = features, job.sharpness = sharpness;
  hipStream_t s = (hipStream_t)stream;
  job.b = block;
  launch_lds<&k_niqe_scale<1>>(dim3(nh * nw), dim3(kNiqeThreads), niqe_lds_bytes<1>(job.b), s, job);
  job.b = block / 2;
  launch_lds<&k_niqe_scale<2>>(dim3(nh * nw), dim3(kNiqeThreads), niqe_lds_bytes<2>(job.b), s, job);
  return check_launch("niqe_features");
}

extern "C" int srk_niqe_features_host(const void* img, int is_u8, const int64_t* strides, int C, int H, int W, int shave,
                                      int block, const double* tables, double* features, double* sharpness) {
  int nh, nw;
  if (int rc = niqe_check(img, tables, features, C, H, W, shave, block, "niqe_features_host", nh, nw)) return rc;
  const NiqeSrc src = niqe_src(img, is_u8, strides, C, H, W, shave);
  const int Hc = nh * block, Wc = nw * block, H2 = Hc / 2, W2 = Wc / 2;
  std::vector<double> P1((size_t)Hc * Wc), V((size_t)H2 * Wc), P2((size_t)H2 * W2);
  for (int y = 0; y < Hc; ++y)
    for (int x = 0; x < Wc; ++x) P1[(size_t)y * Wc + x] = niqe_src_luma(src, y, x);
  for (int i = 0; i < H2; ++i)     // rows first
    for (int x = 0; x < Wc; ++x) {
      double a = 0.0;
      for (int k = 0; k < kNiqeShrinkTaps; ++k)
        a += niqe_shrink_weight(k) * P1[(size_t)niqe_reflect(2 * i - 3 + k, Hc) * Wc + x];
      V[(size_t)i * Wc + x] = a;
    }
  for (int i = 0; i < H2; ++i)     // then columns
    for (int j = 0; j < W2; ++j) {
      double a = 0.0;
      for (int k = 0; k < kNiqeShrinkTaps; ++k)
        a += niqe_shrink_weight(k) * V[(size_t)i * Wc + niqe_reflect(2 * j - 3 + k, Wc)];
      P2[(size_t)i * W2 + j] = a;
    }
  niqe_host_scale(P1, Hc, Wc, block, tables, features, sharpness);
  niqe_host_scale(P2, H2, W2, block / 2, tables, features + SRK_NIQE_FEATURES / 2, nullptr);
  return SRK_OK;
}
