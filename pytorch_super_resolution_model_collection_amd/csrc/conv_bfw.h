// Declarations shared by the wave-specialised persistent convolutions: k_conv_bfw (conv_bfw.hip: two halo buffers, one
// workgroup barrier per stage), k_conv_bfr (conv_bfr.hip: a ring of halo buffers with full / free counters in LDS) and
// k_espcn_pair (conv_pair.hip: the same counters).
#pragma once
#include "srk_common.h"
#include "conv_problem.h"
#include "conv_tile.h"
#include "bf16_frag.h"
#include <stdlib.h>
#include <type_traits>

namespace srk {

// Counters in LDS that the waves of the ring kernels (k_conv_bfr, k_espcn_pair) hand buffers over with.
typedef __attribute__((address_space(3))) unsigned lds_cnt_t;
constexpr unsigned kLdsCntSpinCap = 1u << 18;

__device__ __forceinline__ unsigned lds_cnt_peek(lds_cnt_t* p) {
  return (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
// wait until *p >= target (monotonic counters: the difference stays far below 2^31).  A poll that runs into its cap sets
// `dead`; what a kernel does about it is its own business (k_conv_bfr traps, k_espcn_pair counts).
__device__ __forceinline__ void lds_cnt_wait(lds_cnt_t* p, unsigned target, bool& dead) {
  if (!dead) {
    unsigned spins = 0;
    while ((int)(lds_cnt_peek(p) - target) < 0) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > kLdsCntSpinCap) {
        dead = true;
        break;
      }
    }
  }
  asm volatile("" ::: "memory");
}
// n counts behind every LDS access this wave has issued so far.  No s_waitcnt: the LDS executes the operations of one wave
// in the order they were issued, so whoever sees the count sees the writes (or finds the reads done) that precede it.
__device__ __forceinline__ void lds_cnt_signal(lds_cnt_t* p, unsigned n = 1u) {
  asm volatile("" ::: "memory");
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(p, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  asm volatile("" ::: "memory");
}

constexpr int BFW_MAXTAPS = 32;
constexpr int BFW_IT = 6;  // producer register batches: halos of <= 64 * 6 = 384 pixels

struct BfwParams {
  MfmaConvParams P;
  const uint4* wq;  // prepared filter planes (h, m)
  int ICc, NB, NPIXp, ntiles;
  const float* w_descale;  // F16 kernels: trailer {2^-kw, 2^kw} of the fp16 filter section (wq then points at that section)
  // Output-channel slices: a layer whose whole filter does not fit (64 -> 64: 147 KB) runs as nsl slices of NB = OC / nsl
  // channels; slice sl of tile range i is block 8 * (nsl * i + sl) + xcd -- the nsl blocks that walk the same tiles are
  // neighbours on one XCD and start together, so the halo the first one pulls into that XCD's L2 serves the others.
  int nsl, NBfull, OCb;
  int late;  // consumer waves 4 - 7 park a finished tile at the START of the next stage (see the consumer loop)
  unsigned out_bytes;  // size of the output tensor (buffer descriptor of the consumers' stores)
  int nbuf;  // k_conv_bfr: halo buffers of the ring (3 .. BFR_MAXBUF)
  int cv_kx;  // k_conv_bfr<.., canvas>: patches side by side on the canvas
  int cv_sep;  // ... 1: every cell ends with a separator row / column; 0: patches of whole tiles (H % 8 == 0, W % 16 == 0) stacked
              // without separators -- a halo pixel outside the tile's own patch is padding
  unsigned cv_mh, cv_mw;  // ... ceil(2^32 / (PH + 1)), ceil(2^32 / (PW + 1))
};

// LDS stride (in 16-byte slots) between the four 8-channel groups of a halo plane, chosen against the lane groups the LDS
// serves wide accesses in (MI355X_MICROARCH.md, LDS): ds_read_b128 in {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} / ...
// with bank = slot mod 16, ds_write_b128 in 8 contiguous lanes with a window of 8 slots.
//   producers: 8 lanes write (2 pixels) x (4 groups)          -> conflict-free iff stride = 2 or 6 (mod 8)
//   consumers: a lane group reads 8 columns of k-group kq and the OTHER 8 columns of kq + 1.  With the columns
//     {0-3, 12-15} on the even pixels of the M tile and {4-11} on the odd ones, a stride of +-2 (mod 16) maps a parity
//     class onto itself                                         -> conflict-free for M tiles of 16 consecutive slots
// Measured on the c2 layers (rocprofv3 --pmc SQ_LDS_BANK_CONFLICT): 54.1 M -> 21.9 M conflict cycles
// per launch for 64->32 (0 with 16-wide tiles), 16.2 M -> 0 for 32->48; LDS-busy cycles 139 M -> 107 M.  The layer times
// do not move (0.472 ms either way): the LDS was not what bounds this kernel.
static inline int bfw_group_stride(int npix) {
  const int a = npix + ((2 - npix) & 15), b = npix + ((14 - npix) & 15);
  return a < b ? a : b;
}

// pick_tile (conv_tile.h) with the padded halo size as the fit test
static bool bfw_pick_tile(int maxpix, int PH, int PW, int KHv, int KWv, long cap_px, TilePick& best) {
  bool found = false;
  long best_tiles = 0, best_halo = 0;
  const int maxTW = PW < maxpix ? PW : maxpix;
  for (int TW = 1; TW <= (maxTW > 1 ? maxTW : 1); ++TW) {
    int TH = maxpix / TW;
    if (TH > PH) TH = PH;
    for (; TH >= 1; --TH) {
      const int HH = TH - 1 + KHv, HWd = TW - 1 + KWv;
      if (bfw_group_stride(HH * HWd) > cap_px) continue;
      const long tiles = (long)cdiv(PH, TH) * cdiv(PW, TW);
      const long halo = (long)HH * HWd * tiles;
      const bool fewer = tiles < best_tiles, same = tiles == best_tiles;
      const bool wider = same && halo * 100 <= best_halo * 106 && TW > best.TW;
      const bool smaller = same && halo < best_halo && TW >= best.TW;
      if (!found || fewer || wider || smaller) {
        found = true;
        best_tiles = tiles;
        best_halo = halo;
        best = TilePick{TH, TW, (int)cdiv(PH, TH), (int)cdiv(PW, TW), HH, HWd,
                        (double)PH * PW / ((double)tiles * (double)maxpix)};
      }
      break;  // smaller TH only gets worse for this TW
    }
  }
  return found;
}

// Output-channel slices of a layer (BfwParams.nsl): 1 while the whole filter fits, else 32-channel slices (3x3 only)
static inline int bfw_slices(const GatherConv& g) {
  const int T = g.KH * g.KW;
  if (g.OC <= 48 || (g.OC == 64 && (size_t)T * ((g.IC + 31) / 32) * 8 * g.OC * 16 <= 100 * 1024)) return 1;
  return (T == 9 && g.OC % 32 == 0) ? g.OC / 32 : 0;
}

// conv_bfr.hip: the ring form of the 3x3 kernels with 32 / 48 output channels (per slice); -1 = not applicable
int conv_bfr_launch(const BfwParams& B, hipStream_t s);
// ... and the pair (first layer, 3x3 64 -> 32) as one launch: the first layer computed by the producers (conv_bfr.hip, FUSE)
int conv_bfr_fused(const GatherConv& g1, const float* x, const float* wp1, const Epi& ep1, const GatherConv& g2, const float* wp2,
                   float* out, const Epi& ep2, hipStream_t s);

}  // namespace srk
