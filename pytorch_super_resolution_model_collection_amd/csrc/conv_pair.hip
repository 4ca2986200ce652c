// ESPCN's first two layers in one persistent launch: conv5x5 3 -> 64 + ReLU feeding conv3x3 64 -> 32 + ReLU (both
// "valid", stride 1, f16x3 arithmetic), so the 64-channel map between them never reaches HBM.
//
// One 512-thread block per CU walks a contiguous run of 8 x 16 output tiles of the second layer in column-major order
// (image, tile column, tile row).  Its eight waves form two groups of four (one wave per SIMD each) that take alternate
// tiles of the run.  Every wave computes both layers of its group's tiles: the first layer of tile t+1 into LDS while the
// other group's wave on the same SIMD runs the second layer of tile t out of it.  No wave is a pure loader: the
// 3-channel input tile (14 x 23 px) is loaded, split and staged by the group itself.
//
// The second layer of a tile needs a 10 x 18 halo of the intermediate.  Rows 0 .. 1 of it are rows 8 .. 9 of the tile
// above: a tile whose upper neighbour is the run's previous tile computes only rows 2 .. 9 (144 pixels, nine 16-pixel
// fragments) and takes rows 0 .. 1 from three rotating buffers of kept rows; the first tile of a run and the top tile of a
// column compute their rows 0 .. 1 as three more fragments.  Every value of the intermediate is the same number whichever
// tile computed it (same K order, same scale), so the output does not depend on where runs start.  The coordinates (image,
// tile column, tile row) of a group's tile are split once in front of the tile loop and then advanced by two list steps
// with add and carry; nothing inside the loop divides by a run-time value.
//
// First layer: every one of the 225 products of the f16x3 sum (75 taps x {w_h x_h, w_h x_m, w_m x_h}) has a K slot of
// its own: 256 K in eight 16x16x32 steps, one MFMA per step and channel fragment (pr_kgroup, conv_pair_layout.h).  A
// staged pixel is one 16-byte cell of PQ, {h0 h1 h2 m0 m1 m2 h0 h1}, that meets {wh0 wh1 wh2 wh0 wh1 wh2 wm0 wm1} of a tap: 25 K groups, eight
// of a tap's nine products each; the ninth, wm2 h2, of a kernel row's five taps is one K group against T, which holds h2
// of four pixels in a row per 8-byte cell.  Steps 0 .. 5 read one aligned 16-byte cell per lane, steps 6 and 7 two aligned
// 8-byte halves.  A wave holds the filter side of both 16-channel fragments of ONE 32-channel chunk in registers (64
// VGPRs), so that a pixel fragment read feeds two MFMAs, and computes four of the nine pixel fragments, every other tile
// five.  A cell is requested a K step ahead of its two MFMAs, through five rotating registers of four (l1_frags; DESIGN
// 15.7).  The intermediate's fp16 scale
// is a BOUND, not a measured maximum: max_c(|b_c| + sum |w_c| max|x|) >= max|relu(conv)|, so no rendezvous per tile; a
// power-of-two scale above the true maximum gives the same planes unless the residual plane underflows, i.e. it only
// raises the absolute error floor (ops.declare_absmax).
// Second layer: the ring kernel's tap loop (conv_bfr.hip) with the filter in LDS; a wave owns 4 rows x 16 columns x 16
// channels of the tile.  Accumulation order per output: chunk, kernel column, kernel row.  The second layer's
// MFMA stream is written out with its LDS reads ahead of use: pixel fragments two steps ahead, across the chunk boundary
// too, filter fragments replaced behind their last use.
//
// Ring: stage (run entry i, chunk c) = 2 i + c holds halo rows 2 .. 7 in slot (2 i + c) % 3; per slot full / free counters
// in LDS.  A wave waits for free >= 4 k before writing use k of a slot and for full >= 2 (k + 1) (the two waves of the
// chunk) before reading it, and signals free right behind its last read of a slot.  Halo rows 8 .. 9 go to a kept-row
// buffer with counters of its own (see the tile loop).  Every poll is capped: a slip is counted (srk_ring_timeouts) and
// the waves run on with wrong numbers instead of faulting the device.
//
// max|x| (the input's scale, and through the bound the intermediate's) is either handed in (x_amax of a producer, of
// srk_absmax or declared) or measured inside the launch: block b of G reduces the float4 slice [b n / G, (b + 1) n / G)
// of x, raises slot b % 16 with one atomic, waits for it to return and arrives on a counter word of the slots buffer; after the rest of its
// prologue its first wave polls for G arrivals (capped) and reads the slots.  Departures are counted beside the arrivals and
// the last block to leave zeroes both words, so a captured launch replays.  A block whose poll runs into its cap scans all
// of x itself (counted in srk_espcn_pair_scans, not in srk_ring_timeouts).  Maximum is order-free and only its exponent is
// used, so the output is the same bits either way.
//
// Everything that depends on the first layer's filter alone -- the fp16 planes of every lane's fragments, sum |w_c|, |b_c|,
// the filter's maximum -- is prepared once per filter by k_espcn_pair_prep with the same device functions; the kernel
// loads 16 words per lane.
//
// Dead rows: a column's last tile has vr = OH - 8 ty live output rows.  Output row r reads halo rows r .. r + 2, so halo
// rows >= vr + 2 reach nothing that is stored.  Fragment f of rows 2 .. 9 starts in halo row (36 + 16 f) / 18: the waves of
// pixel half 1 (f >= 4, first row 5) skip their first layer when vr <= 3, the waves of output rows 4 .. 7 their second layer
// and stores when vr <= 4.  They still perform every wait and signal.
#include "conv_bfw.h"   // lds_cnt_*; srk_common.h, conv_problem.h, bf16_frag.h
#include "conv_pair_layout.h"   // the staged tile, pr_kgroup, the fragment addresses (shared with tools/pair_lds_host_check.cpp)

namespace srk {

namespace {

constexpr int PR_TH = 8, PR_TW = 16;
constexpr int PR_NSLOTPIX = 6 * PR_HW, PR_NPIXP = PR_NSLOTPIX + 2;  // halo rows 2 .. 7 live in a ring slot: pixels, stride
                                                                    // (pixel p of rows 2 .. 9 is halo pixel 36 + p)
constexpr int PR_KP = PR_NKEEP + 2;                 // halo rows 8 .. 9 = the tile below's rows 0 .. 1 (PR_NKEEP pixels): stride
constexpr int PR_NSLOT = 3, PR_NKBUF = 3;
constexpr int PR_WL2 = 9 * 2 * 256;                 // uint4 of the second layer's filter [tap][chunk][plane][group][32]
constexpr int PR_HBUF = 4 * PR_NPIXP;               // uint4 per plane of a halo slot [group][NPIXP]
constexpr int PR_KBUF = 2 * 4 * PR_KP;              // uint4 per plane of a kept-row buffer [chunk][group][KP]
constexpr int PR_PLANE = PR_NSLOT * PR_HBUF + PR_NKBUF * PR_KBUF;   // the residual planes of all of them lie this far on
constexpr unsigned PR_AMAX_CAP = 1u << 14;          // polls of the max|x| rendezvous (one L2 round trip and a sleep each)
constexpr int PR_ARRIVE = 1, PR_DEPART = 2;         // counter words of the slots buffer (slot i is word 16 i)
// Both words MUST stay in one 64-byte line and be touched by one thread of a block (thread 0).  The reset -- the last
// block to leave zeroes both -- needs every block's arrival, an atomic without a return value, to be performed before
// that block's own later departure.  Nothing in the memory model orders two relaxed atomics on different words; what
// does is the hardware path: a wave's vector memory instructions leave the CU in issue order, an address selects its L2
// channel by line, so both requests queue at the same channel behind each other, and device-scope atomics on ordinary
// device memory (what the slots are: a torch allocation) are performed there.  Moved to different lines, or issued by different
// waves, the arrival could land after the zeroing and leave the counter at 1 for the next launch.  The ordering of a
// block's slot maximum before its arrival does not lean on this: the maximum returns a value the arrival waits for.
// l1_frags requests the cell of group g + D in front of the MFMAs of group g: a K step ahead in the two- and the four-
// fragment form; the five-fragment form, where the kernel's register maximum lies, keeps the same five cell registers
#define PR_L1_AHEAD(NM) ((NM) == 2 ? 2 : 4)
constexpr int PR_XLD = 24;                          // float4 loads a thread keeps in flight over its part of the slice
constexpr int PR_W1P = 2 * 2 * 8 * 64;              // uint4 of the prepared first layer [c1][nf][ks][lane]; behind
constexpr int PR_W1P_FLOATS = 144;                  // them floats: sum |w_c| [64], |b_c| [64], max |w|
constexpr size_t PR_W1P_BYTES = (size_t)PR_W1P * 16 + PR_W1P_FLOATS * 4;
constexpr size_t PR_LDS = (size_t)PR_WL2 * 16 + (size_t)2 * PR_PLANE * 16 + (size_t)2 * PR_XBUF + 64;
static_assert(PR_LDS <= 160 * 1024, "k_espcn_pair: LDS");

__device__ unsigned g_pair_timeouts = 0;
__device__ unsigned g_pair_scans = 0;   // blocks that scanned all of x themselves (rendezvous cap, or asked for)

typedef unsigned v4u_t __attribute__((ext_vector_type(4)));

struct PairParams {
  const float* x;          // NCHW [N][3][H][W]
  const uint4* w1p;        // the first layer as k_espcn_pair_prep leaves it
  const float* b1;         // [64]
  const uint4* wq2;        // fp16 section of the second layer's prepared filter
  const float* w2_descale; // its trailer {2^-kw, 2^kw}
  const float* b2;         // [32]
  float* y;                // NHWC [N][H-6][W-6][32]
  float* x_amax;           // slots of max|x|: read (amax_mode 0) or raised here
  float* y_amax;
  size_t xn;               // elements of x
  int amax_mode;           // 0: x_amax holds the maximum; 1: measured in this launch; 2: same, every block scans all of x
  int N, H, W, OH, OW, tiles_x, tiles_y, img_tiles, ntiles;
  unsigned x_img_bytes, y_bytes;
};

// max |x| over the float4s [lo, hi) (thread t of nt takes lo + t, lo + t + nt, ..: PR_XLD loads in flight) and, with `tail`,
// over the elements behind the last whole float4
__device__ __forceinline__ float pr_slice_absmax(const float* __restrict__ x, size_t lo, size_t hi, size_t n, bool tail,
                                                 int t, int nt) {
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  float m = 0.f;
  for (size_t base = lo; base < hi; base += (size_t)nt * PR_XLD) {
    f32x4 v[PR_XLD];
#pragma unroll
    for (int k = 0; k < PR_XLD; ++k) {
      const size_t e = base + (size_t)t + (size_t)k * nt;
      v[k] = x4[e < hi ? e : hi - 1];
    }
#pragma unroll
    for (int k = 0; k < PR_XLD; ++k) m = abs_max4(m, v[k]);
  }
  if (tail) {
    const size_t e = (n & ~(size_t)3) + (size_t)t;
    if (t < 3 && e < n) m = fmaxf(m, fabsf(x[e]));
  }
  return m;
}

// The first layer's filter as the lanes of k_espcn_pair hold it: wave c1 of two writes, for its 32-channel chunk, lane
// `lane`'s filter side of channel fragment nf and K group (ks, kq) at the filter's scale; wave 0 adds sum |w_c|, |b_c| and
// the filter's maximum.
__global__ __launch_bounds__(128) void k_espcn_pair_prep(const float* __restrict__ w1, const float* __restrict__ b1,
                                                         uint4* __restrict__ out) {
  const int lane = threadIdx.x & 63, c1 = threadIdx.x >> 6;
  const int j = lane & 15, kq = lane >> 4;
  float wsum = 0.f, wmax = 0.f;
  {
    const float* wc = w1 + lane * 75;
    for (int i = 0; i < 75; ++i) {
      const float a = fabsf(wc[i]);
      wsum += a;
      wmax = fmaxf(wmax, a);
    }
  }
  const float wm = wave_max(wmax);
  const float sw1 = exp2i(amax_scale_exp(wm));
#pragma unroll
  for (int nf = 0; nf < 2; ++nf) {
    const int co = c1 * 32 + nf * 16 + j;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const PrKGroup g = pr_kgroup(ks, kq);
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool tap = g.kind == PR_KTAP;
        const bool on = tap || (g.kind == PR_KROW && e < 5);   // (the load's index stays inside w1 either way)
        const int ci = tap ? (e < 6 ? e % 3 : e - 6) : 2, dx = tap ? g.dx : (e < 5 ? e : 0);
        f[e] = on ? w1[((co * 3 + ci) * 5 + g.dy) * 5 + dx] : 0.f;
      }
      uint4 pl[2];
      split8h(f, sw1, pl);
      out[((c1 * 2 + nf) * 8 + ks) * 64 + lane] = g.kind == PR_KTAP ? make_uint4(pl[0].x, pl[0].y, pl[0].z, pl[1].w) : pl[1];
    }
  }
  if (c1 == 0) {
    float* t = reinterpret_cast<float*>(out + PR_W1P);
    t[lane] = wsum;
    t[64 + lane] = fabsf(b1[lane]);
    if (lane == 0) t[128] = wm;
  }
}

__global__ __launch_bounds__(512, 1) void k_espcn_pair(PairParams B) {
  extern __shared__ __attribute__((aligned(16))) uint4 smem4[];
  uint4* wl2 = smem4;
  uint4* ring = smem4 + PR_WL2;
  uint4* keep = ring + PR_NSLOT * PR_HBUF;
  unsigned char* xin_all = reinterpret_cast<unsigned char*>(ring + 2 * PR_PLANE);
  lds_cnt_t* cnt = (lds_cnt_t*)(xin_all + 2 * PR_XBUF);  // full[3], free[3], staged[2], kept full[3], kept free[3]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = wave >> 2, gw = wave & 3, lt = tid & 255;
  const int j = lane & 15, kq = lane >> 4;
  unsigned char* xin = xin_all + grp * PR_XBUF;   // the group's PQ, T PR_XT bytes on

  // ---- max|x|: handed in, or this block's slice of it on its way to the slots (the other blocks' comes back below) --------
  const float* w1t = reinterpret_cast<const float*>(B.w1p + PR_W1P);   // sum |w_c| [64], |b_c| [64], max |w|
  const int nblk = gridDim.x;
  float xmax = 0.f;
  if (tid < 14) cnt[tid] = 0u;
  if (B.amax_mode) {
    float* red = reinterpret_cast<float*>(xin_all);   // (free until the first tile is staged)
    const size_t n4 = B.xn >> 2;
    const float m = wave_max(pr_slice_absmax(B.x, (size_t)blockIdx.x * n4 / nblk, (size_t)(blockIdx.x + 1) * n4 / nblk, B.xn,
                                             blockIdx.x == 0, tid, 512));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    if (tid == 0) {
      float b = red[0];
#pragma unroll
      for (int i = 1; i < 8; ++i) b = fmaxf(b, red[i]);
      // The arrival is issued once the maximum has RETURNED, i.e. has been performed where agent-scope atomics are (beyond
      // the XCD's L2); the readers use agent-scope atomic loads.  No fence: at agent scope it writes back and invalidates
      // the XCD's L2, which cost the rendezvous 10 us.
      const unsigned was = atomicMax(reinterpret_cast<unsigned*>(B.x_amax + (blockIdx.x & 15) * 16), __float_as_uint(b));
      asm volatile("s_waitcnt vmcnt(0)" ::"v"(was) : "memory");
      __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(B.x_amax) + PR_ARRIVE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  } else {
    xmax = amax_read(B.x_amax);
  }

  // ---- second layer's filter into LDS: a thread's nine loads in flight before its first LDS store (as a plain loop they are
  // nine L2 round trips in a row, conv_bfr.hip) -------------------------------------------------------------------------
  {
    static_assert(PR_WL2 == 9 * 512, "k_espcn_pair: filter copy");
    v4u_t wv[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) wv[i] = *reinterpret_cast<const v4u_t*>(B.wq2 + tid + 512 * i);
#pragma unroll
    for (int i = 0; i < 9; ++i) *reinterpret_cast<v4u_t*>(wl2 + tid + 512 * i) = wv[i];
  }

  // ---- first layer: chunk c1 = channels 32 c1 .. 32 c1 + 31 as two 16-channel fragments, half mh of the pixel fragments -----
  // filter fragments: channel 32 c1 + 16 nf + j, K group (ks, kq) (prepared: k_espcn_pair_prep)
  const int c1 = gw >> 1, mh = gw & 1;
  const int mhu = __builtin_amdgcn_readfirstlane(mh), rhu = __builtin_amdgcn_readfirstlane(gw >> 1);  // (dead-row branches)
  uint4 w1f[2][8];  // [channel fragment][K step]
#pragma unroll
  for (int nf = 0; nf < 2; ++nf)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) w1f[nf][ks] = B.w1p[((c1 * 2 + nf) * 8 + ks) * 64 + lane];
  const float wsum = w1t[lane], babs = w1t[64 + lane];
  // Rows 2 .. 9 of the halo are nine 16-pixel fragments, pixel 16 f + j of the 144: the wave takes f = 4 mh + m, m < 4, and
  // every other own tile the ninth as m = 4.  Rows 0 .. 1 (36 pixels) are three fragments: f = 2 mh + m, m < 2.  Lane
  // column j holds pixel PR_FPIX(j) of its fragment (which pixels share a 16-lane group of ds_read_b128: DESIGN 15.5).
  // Offsets in staged cells: fragment -> the pixel's cell kq columns on (the top ones clamped to pixel 35).  K steps 0 .. 4
  // read PQ cell offset + ks PR_XP, step 5 offset + k5; step s of 6 and 7 reads two 8-byte halves, at byte offset * kmul[s]
  // + kadd[s] and kd[s] on: of the PQ cell of tap (4, 4) or of T's cells of the lane's row.  A lane without a K group reads
  // what its neighbour reads (the same addresses cost no LDS cycle).
  // (conv_pair_layout.h holds these expressions: pr_body_pix, pr_top_pix, pr_cell_off, pr_k5, pr_k67)
  int mpix[5], moff[5], tpix[2], toff[2];
#pragma unroll
  for (int m = 0; m < 5; ++m) {
    mpix[m] = pr_body_pix(mh, m, j) - PR_NKEEP;
    moff[m] = pr_cell_off(pr_body_pix(mh, m, j), kq);
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    tpix[m] = 16 * (2 * mh + m) + pr_fpix(j);
    toff[m] = pr_cell_off(pr_top_pix(mh, m, j), kq);
  }
  const int k5 = pr_k5(kq);
  int kmul[2], kadd[2], kd[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const PrK67 k = pr_k67(s, kq);
    kmul[s] = k.kmul;
    kd[s] = k.kd;
    asm volatile("" : "+v"(kd[s]));   // (step 7's is 32 in every lane: as a constant the two reads become one ds_read2_b64)
    kadd[s] = k.kadd;
  }
  // where this lane's four channels of fragment 0 go: byte offset of pixel 0 inside a slot / inside a buffer of kept rows
  // (fragment 1: two 8-channel groups on)
  const int wr_slot = (kq >> 1) * PR_NPIXP * 16 + (kq & 1) * 8, wr_keep = (c1 * 4 + (kq >> 1)) * PR_KP * 16 + (kq & 1) * 8;

  // ---- second layer: rows 4 rh .. 4 rh + 3, channels 16 nf2 .. 16 nf2 + 15 -------------------------------------------
  // Halo row 4 rh + R is slot row 4 rh + R - 2, except halo rows 0 .. 1 (rh == 0: R = 0, 1) and 8 .. 9 (rh == 1: R = 4, 5),
  // which are kept rows.
  const int rh = gw >> 1, nf2 = gw & 1;
  const int pj = j < 4 ? 2 * j : (j < 12 ? 2 * j - 7 : 2 * j - 16);
  const int lane_b = (4 * rh - 2) * PR_HW + pj + kq * PR_NPIXP;
  const int lane_k = pj + kq * PR_KP;
  const int lane_a = kq * 32 + nf2 * 16 + j;
  float b2v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) b2v[e] = B.b2[nf2 * 16 + 4 * kq + e];

  // ---- tiles of this block: a contiguous run of the column-major order (image, tile column, tile row), runs of equal
  // length +-1; the blocks of an XCD take neighbouring runs ------------------------------------------------------------
  const int xcd = blockIdx.x & 7;
  int first, count;
  {
    const int lb = xcd * (nblk >> 3) + (xcd < (nblk & 7) ? xcd : (nblk & 7)) + (blockIdx.x >> 3);
    const int per = B.ntiles / nblk, rem = B.ntiles - per * nblk;
    first = lb * per + (lb < rem ? lb : rem);
    count = per + (lb < rem ? 1 : 0);
  }
  count = __builtin_amdgcn_readfirstlane(count);
  // Tile coordinates (image, tile column, tile row) of the group's current tile, the same in every lane of a wave, split
  // once here (the only divisions by run-time values) and advanced by two list steps with add and carry (conv_bfr.hip's
  // adv2; as two single steps, so that no step vector is held): the tile two on is the group's next, whose input xload
  // fetches.  Held in VGPRs: as SGPRs they turn the tile loop's tests into scalar branches and cost six SGPR spills.
  int cn, cx, cy;
  {
    const int t = first + grp;
    const int n = t / B.img_tiles, rem = t - n * B.img_tiles, x = rem / B.tiles_y;
    cn = n;
    cx = x;
    cy = rem - x * B.tiles_y;
  }
  auto adv2 = [&](int& n, int& x, int& y) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (++y == B.tiles_y) {
        y = 0;
        if (++x == B.tiles_x) {
          x = 0;
          ++n;
        }
      }
    }
  };

  const __amdgpu_buffer_rsrc_t yr = buffer_rsrc(B.y, B.y_bytes);
  const unsigned HW_ = (unsigned)(B.H * B.W);
  // input staging: pixel q = lt + 256 s of the 14 x 23 tile, 3 channels
  float xv[2][3];
  auto xload = [&](int i, int n, int tx, int ty) {   // run entry i = tile (n, tx, ty); nothing is read past the run's end
    const bool valid = i < count;
    const __amdgpu_buffer_rsrc_t xr = buffer_rsrc(B.x + (size_t)(valid ? n : 0) * 3 * HW_, B.x_img_bytes);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int q = lt + 256 * s, qy = q / PR_XC, qx = q - qy * PR_XC;
      const bool ok = valid && q < PR_XR * PR_XC;
      const unsigned o = ok ? 4u * (unsigned)((ty * PR_TH + qy) * B.W + tx * PR_TW + qx) : 0x80000000u;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        xv[s][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, (int)(o + (ok ? 4u * c * HW_ : 0u)), 0, 0));
    }
  };
  // NM 16-pixel fragments of the first layer (per output: K step order 0 .. 7, one product per step).  A group is one cell
  // and its two MFMAs, groups run in the order (K step, fragment); the cell of group g + D is requested in front of the
  // MFMAs of group g, through D + 1 rotating registers of four: a K step ahead where the registers allow it.
  auto l1_frags = [&](auto nm, const int* off, f32x4 (*a)[2]) {
    constexpr int NM = decltype(nm)::value, G = 8 * NM, D = PR_L1_AHEAD(NM);
    uint4 xc[D + 1];
    auto rd = [&](auto gc) {
      constexpr int g = decltype(gc)::value, ks = g / NM, m = g % NM;
      if constexpr (ks < 6) {
        xc[g % (D + 1)] = *reinterpret_cast<const uint4*>(xin + 16 * (off[m] + (ks < 5 ? ks * PR_XP : k5)));
      } else {
        const int pa = __mul24(off[m], kmul[ks & 1]) + kadd[ks & 1];
        const uint2 ca = *reinterpret_cast<const uint2*>(xin + pa), cb = *reinterpret_cast<const uint2*>(xin + pa + kd[ks & 1]);
        xc[g % (D + 1)] = make_uint4(ca.x, ca.y, cb.x, cb.y);
      }
    };
#pragma unroll
    for (int m = 0; m < NM; ++m) a[m][0] = a[m][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    srk_static_for<0, D>([&](auto gc) { rd(gc); });
    __builtin_amdgcn_sched_barrier(0);
    srk_static_for<0, G>([&](auto gc) {
      constexpr int g = decltype(gc)::value, ks = g / NM, m = g % NM;
      if constexpr (g + D < G) rd(std::integral_constant<int, g + D>{});
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) a[m][nf] = mfma16h(w1f[nf][ks], xc[g % (D + 1)], a[m][nf]);
      __builtin_amdgcn_sched_barrier(0);
    });
  };
  bool dead = false;
  float amax = 0.f;
  xload(grp, cn, cx, cy);
  // ---- max|x| of all blocks: the first wave polls for their arrivals, reads the slots, leaves (the last one to leave
  // zeroes the two counter words: a captured launch replays) ---------------------------------------------------------------
  if (B.amax_mode && wave == 0) {
    unsigned* ctr = reinterpret_cast<unsigned*>(B.x_amax);
    bool late = B.amax_mode == 2;
    if (!late) {
      unsigned spins = 0;
      while ((int)((unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(ctr + PR_ARRIVE, __ATOMIC_RELAXED,
                                                                                   __HIP_MEMORY_SCOPE_AGENT)) -
                   (unsigned)nblk) < 0) {
        __builtin_amdgcn_s_sleep(16);
        if (++spins > PR_AMAX_CAP) {
          late = true;
          break;
        }
      }
    }
    asm volatile("" ::: "memory");
    // agent-scope atomic loads, served where the atomics land (amax_peek); issued behind the poll that saw the last arrival
    const float sv = wave_max(__hip_atomic_load(B.x_amax + (lane & 15) * 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (lane == 0) {
      cnt[14] = __float_as_uint(sv);
      cnt[15] = late ? 1u : 0u;
      const unsigned d = __hip_atomic_fetch_add(ctr + PR_DEPART, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (d + 1u == (unsigned)nblk) {   // every block has arrived and finished polling
        __hip_atomic_store(ctr + PR_ARRIVE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ctr + PR_DEPART, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  __syncthreads();  // filter, counters and max|x| visible
  if (B.amax_mode) {
    xmax = __uint_as_float(lds_cnt_peek(cnt + 14));
    if (lds_cnt_peek(cnt + 15)) {
      // The slots may lack a block that has not arrived: scan all of x here.  (With the slots, which hold every earlier
      // launch's maximum, that is the running maximum the other blocks see.)
      float* red = reinterpret_cast<float*>(xin_all);
      const float m = wave_max(pr_slice_absmax(B.x, 0, B.xn >> 2, B.xn, true, tid, 512));
      if (lane == 0) red[wave] = m;
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 8; ++i) xmax = fmaxf(xmax, red[i]);
      xmax = __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint(xmax)));
      __syncthreads();
      if (tid == 0) atomicAdd(&g_pair_scans, 1u);
    }
  }
  // The staged tiles start out as zeros (red was in there): T's last slots of a row belong to pixels nobody stages, and the
  // zero weights they and the empty K groups meet need a finite partner.
  for (int i = tid; i < 2 * PR_XBUF / 16; i += 512) reinterpret_cast<uint4*>(xin_all)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  // ---- scales: input (its maximum), first-layer filter (its maximum), intermediate (bound) --------------------------
  const int kx = amax_scale_exp(xmax);
  const float bnd = wave_max(fabsf(babs) + wsum * xmax);
  const int kw1 = amax_scale_exp(w1t[128]);
  const int km = amax_scale_exp(bnd);
  const float sx1 = exp2i(kx), sxm = exp2i(km);
  const float dsc1 = exp2i(-kx) * exp2i(-kw1);
  const float dsc2 = exp2i(-km) * B.w2_descale[0];

  unsigned own = 0;  // own tiles done
  unsigned kseq = 0;
  int typrev = 0;
  for (int i = grp; i < count; i += 2, ++own) {
    const int n = cn, tx = cx, ty = cy;
    adv2(cn, cx, cy);   // (the next own tile's)
    // Rows 0 .. 1 of this tile's halo are rows 8 .. 9 of the tile above when that is the run's previous tile; the first
    // tile of a run and a column's top tile compute them.  Kept rows are numbered along the run: a tile's rows 8 .. 9 are
    // number kseq, its rows 0 .. 1 number kseq - 1 (the previous tile's kseq, or a number of their own when computed
    // here); number q lives in buffer q % 3 as its use q / 3.  Every number is written once by the four waves of one
    // group and released eight times: by the four waves of the tile whose rows 8 .. 9 it is and by those of the tile
    // below, or twice by the former when no tile takes it over (and twice by the tile that computed its own rows 0 .. 1).
    // A buffer comes round after three numbers, so in the steady state its readers are two tiles behind the writer.
    const bool fresh = i == 0 || ty == 0;
    const bool hand = i + 1 < count && ty + 1 < B.tiles_y;
    kseq = i == grp ? (grp == 0 ? 1u : 2u + (ty == 0 ? 1u : 0u))
                    : kseq + 2u + (typrev + 1 == B.tiles_y ? 1u : 0u) + (ty == 0 ? 1u : 0u);
    typrev = ty;
    const unsigned kb = kseq % PR_NKBUF, ku = kseq / PR_NKBUF, tb = (kseq - 1u) % PR_NKBUF, tu = (kseq - 1u) / PR_NKBUF;
    // -- stage the input tile (split into fp16 planes at the input's scale), fetch the next own tile's ---------------
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int q = lt + 256 * s;
      if (q < PR_XR * PR_XC) {
        const int qy = q / PR_XC, qx = q - qy * PR_XC;
        unsigned h01, m01, h2, m2;
        split2h(xv[s][0], xv[s][1], sx1, h01, m01);
        split2h(xv[s][2], 0.f, sx1, h2, m2);   // (high halves: zero)
        *reinterpret_cast<uint4*>(xin + 16 * (qy * PR_XP + qx)) = make_uint4(h01, h2 | (m01 << 16), (m01 >> 16) | (m2 << 16), h01);
        // h2 into slot k of T(qy, qx - k): the four cells that start at most three pixels to the left.  Unpredicated: left
        // of column 0 that is columns 21 .. 23 of the row above, in slots that meet zero weights or nothing (one slot per
        // such cell, this thread's alone).
        unsigned short* tq = reinterpret_cast<unsigned short*>(xin + PR_XT) + 4 * (qy * PR_XP + qx);
#pragma unroll
        for (int k = 0; k < 4; ++k) tq[-3 * k] = (unsigned short)h2;
      }
    }
    lds_cnt_signal(cnt + 6 + grp);
    xload(i + 2, cn, cx, cy);
    lds_cnt_wait(cnt + 6 + grp, 4u * (own + 1), dead);

    float b1v[2][4];  // (read per tile: registers are short where the second layer runs)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int e = 0; e < 4; ++e) b1v[nf][e] = B.b1[c1 * 32 + nf * 16 + 4 * kq + e];
    // bias, ReLU, split at the intermediate's scale; the (high, residual) plane words of the lane's 2 x 4 channels of one
    // pixel go to pixel cell `pix` of a [group][pitch] block of 16-byte cells and of its residual twin PR_PLANE cells on
    auto l1_store = [&](const f32x4 (&a)[2], unsigned char* base, int pix, int pitch) {
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(__builtin_fmaf(a[nf][e], dsc1, b1v[nf][e]), 0.f);
        unsigned h01, m01, h23, m23;
        split2h(v[0], v[1], sxm, h01, m01);
        split2h(v[2], v[3], sxm, h23, m23);
        *reinterpret_cast<uint2*>(base + ((2 * nf) * pitch + pix) * 16) = make_uint2(h01, h23);
        *reinterpret_cast<uint2*>(base + (PR_PLANE + (2 * nf) * pitch + pix) * 16) = make_uint2(m01, m23);
      }
    };
    // -- first layer: this wave's fragments of rows 2 .. 9, the 32 channels of its chunk, into the ring -----------------
    auto l1_tile = [&](auto nm) {
      constexpr int NM = decltype(nm)::value;
      f32x4 a1[NM][2];
      l1_frags(nm, moff, a1);
      const unsigned st = 2u * (unsigned)i + c1, slot = st % PR_NSLOT, use = st / PR_NSLOT;
      unsigned char* hb = reinterpret_cast<unsigned char*>(ring + slot * PR_HBUF) + wr_slot;
      lds_cnt_wait(cnt + 3 + slot, 4u * use, dead);
#pragma unroll
      for (int m = 0; m < NM; ++m)
        if (mpix[m] < PR_NSLOTPIX) l1_store(a1[m], hb, mpix[m], PR_NPIXP);
      lds_cnt_signal(cnt + slot);
      // rows 8 .. 9 = pixels 108 .. 143 (in fragments 6 .. 8, m >= 2 where a wave has them) are kept rows
      unsigned char* kp = reinterpret_cast<unsigned char*>(keep + kb * PR_KBUF) + wr_keep;
      lds_cnt_wait(cnt + 11 + kb, 8u * ku, dead);
#pragma unroll
      for (int m = 2; m < NM; ++m)
        if (mpix[m] >= PR_NSLOTPIX) l1_store(a1[m], kp, mpix[m] - PR_NSLOTPIX, PR_KP);
      lds_cnt_signal(cnt + 8 + kb);
    };
    // Live rows of this tile; halo rows >= vr + 2 reach no stored value (file header).  A wave whose fragments all lie there
    // -- pixel half 1 starts in halo row 5 -- only keeps the counters going.
    const int vr = B.OH - ty * PR_TH;
    if (mhu == 1 && vr <= 3) {
      const unsigned st = 2u * (unsigned)i + c1, slot = st % PR_NSLOT, use = st / PR_NSLOT;
      lds_cnt_wait(cnt + 3 + slot, 4u * use, dead);
      lds_cnt_signal(cnt + slot);
      lds_cnt_wait(cnt + 11 + kb, 8u * ku, dead);
      lds_cnt_signal(cnt + 8 + kb);
    } else if (mh == (int)(own & 1)) {
      l1_tile(std::integral_constant<int, 5>{});
    } else {
      l1_tile(std::integral_constant<int, 4>{});
    }
    if (fresh) {  // rows 0 .. 1 computed here
      f32x4 at[2][2];
      l1_frags(std::integral_constant<int, 2>{}, toff, at);
      unsigned char* kp = reinterpret_cast<unsigned char*>(keep + tb * PR_KBUF) + wr_keep;
      lds_cnt_wait(cnt + 11 + tb, 8u * tu, dead);
#pragma unroll
      for (int m = 0; m < 2; ++m)
        if (tpix[m] < PR_NKEEP) l1_store(at[m], kp, tpix[m], PR_KP);
      lds_cnt_signal(cnt + 8 + tb);
    }

    // -- second layer out of the ring and the kept rows --------------------------------------------------------------
    lds_cnt_wait(cnt + 8 + (rh == 0 ? tb : kb), 4u * ((rh == 0 ? tu : ku) + 1u), dead);
    if (rhu == 1 && vr <= 4) {  // output rows 4 .. 7 lie below the output: waits and signals only
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const unsigned st = 2u * (unsigned)i + cc, slot = st % PR_NSLOT, use = st / PR_NSLOT;
        lds_cnt_wait(cnt + slot, 2u * (use + 1), dead);
        lds_cnt_signal(cnt + 3 + slot);
      }
      lds_cnt_signal(cnt + 11 + tb, fresh ? 2u : 1u);
      lds_cnt_signal(cnt + 11 + kb, hand ? 1u : 2u);
    } else {
      f32x4 acc[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
      // The tap loop as a written-out stream (conv_bfr.hip's): 18 steps (kernel column v, halo row R) per chunk, a step's
      // MFMA groups in ascending kernel row.  Behind a step's first group: the pixel fragment of step s + 2 -- from step 16
      // of chunk 0 on that of chunk 1, whose counter is peeked at step 8 and checked at step 16, behind the hand-back of
      // chunk 0's slot at step 15 (a wave never holds a slot while it waits for another) -- and one kernel row of filter
      // fragments: row 0 follows at R = 4 and row 1 at R = 5 (next column, or chunk 1's first), row 2 at R = 0 of the column
      // that needs it at R = 2.  Sums and their order are the plain loop's.
      uint4 fa[3][2], fb[3][2];
      const uint4 *spa[2], *shb[2], *spc[2];
      unsigned sslot[2], suse[2];
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const unsigned st = 2u * (unsigned)i + cc;
        sslot[cc] = st % PR_NSLOT;
        suse[cc] = st / PR_NSLOT;
        shb[cc] = ring + sslot[cc] * PR_HBUF + lane_b;
        // the wave's rows out of kept rows: R = 0, 1 (rh == 0: rows 0 .. 1), R = 4, 5 (rh == 1: rows 8 .. 9)
        const uint4* kr = keep + (rh == 0 ? tb : kb) * PR_KBUF + cc * 4 * PR_KP + lane_k - (rh == 0 ? 0 : 4 * PR_HW);
        spa[cc] = rh == 0 ? kr : shb[cc];
        spc[cc] = rh == 0 ? shb[cc] : kr;
      }
      auto ldA = [&](auto uc, auto vc, auto ccc) {
        constexpr int u = decltype(uc)::value, v = decltype(vc)::value, cc = decltype(ccc)::value;
        fa[u][0] = wl2[((u * 3 + v) * 2 + cc) * 256 + lane_a];
        fa[u][1] = wl2[((u * 3 + v) * 2 + cc) * 256 + 128 + lane_a];
      };
      auto ldB = [&](auto ccc, auto sc) {
        constexpr int cc = decltype(ccc)::value, s = decltype(sc)::value, v = s / 6, R = s - 6 * v;
        const uint4* px = R < 2 ? spa[cc] : (R < 4 ? shb[cc] : spc[cc]);
        fb[s % 3][0] = px[R * PR_HW + v];
        fb[s % 3][1] = px[R * PR_HW + v + PR_PLANE];
      };
      using I0 = std::integral_constant<int, 0>;
      using I1 = std::integral_constant<int, 1>;
      using I2 = std::integral_constant<int, 2>;
      lds_cnt_wait(cnt + sslot[0], 2u * (suse[0] + 1), dead);
      ldA(I0{}, I0{}, I0{});
      ldB(I0{}, I0{});
      ldA(I1{}, I0{}, I0{});
      ldB(I0{}, I1{});
      srk_static_for<0, 2>([&](auto ccc) {
        constexpr int cc = decltype(ccc)::value;
        unsigned peek_v = 0;
        srk_static_for<0, 18>([&](auto sc) {
          constexpr int s = decltype(sc)::value, v = s / 6, R = s - 6 * v;
          constexpr int u_lo = R - 3 > 0 ? R - 3 : 0, u_hi = R < 2 ? R : 2;
          srk_static_for<u_lo, u_hi + 1>([&](auto uc) {
            constexpr int u = decltype(uc)::value, r = R - u;
            acc[r] = mfma16h(fa[u][0], fb[s % 3][1], acc[r]);
            acc[r] = mfma16h(fa[u][1], fb[s % 3][0], acc[r]);
            acc[r] = mfma16h(fa[u][0], fb[s % 3][0], acc[r]);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (u == u_lo) {
              if constexpr (cc == 0 && s == 16) {
                if (!dead) {
                  unsigned seen = (unsigned)__builtin_amdgcn_readfirstlane((int)peek_v), spins = 0;
                  while ((int)(seen - 2u * (suse[1] + 1)) < 0) {
                    __builtin_amdgcn_s_sleep(1);
                    seen = lds_cnt_peek(cnt + sslot[1]);
                    if (++spins > kLdsCntSpinCap) {
                      dead = true;
                      break;
                    }
                  }
                }
                asm volatile("" ::: "memory");
              }
              if constexpr (s + 2 < 18) ldB(ccc, std::integral_constant<int, s + 2>{});
              else if constexpr (cc == 0) ldB(I1{}, std::integral_constant<int, s + 2 - 18>{});
              if constexpr (cc == 0 && s == 8)
                peek_v = __hip_atomic_load(cnt + sslot[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              if constexpr (s == 15) lds_cnt_signal(cnt + 3 + sslot[cc]);   // behind the slot's last read (step 17's)
              __builtin_amdgcn_sched_barrier(0);
              if constexpr (R == 0) {
                ldA(I2{}, std::integral_constant<int, v>{}, ccc);
                __builtin_amdgcn_sched_barrier(0);
              } else if constexpr (R >= 4) {
                if constexpr (v < 2) ldA(std::integral_constant<int, R - 4>{}, std::integral_constant<int, v + 1>{}, ccc);
                else if constexpr (cc == 0) ldA(std::integral_constant<int, R - 4>{}, I0{}, I1{});
                __builtin_amdgcn_sched_barrier(0);
              }
            }
          });
        });
      });
      lds_cnt_signal(cnt + 11 + tb, fresh ? 2u : 1u);
      lds_cnt_signal(cnt + 11 + kb, hand ? 1u : 2u);
      // -- epilogue: bias, ReLU, NHWC stores of the pixels inside the output, running maximum -----------------------------
      const int oc = tx * PR_TW + pj;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int orow = ty * PR_TH + 4 * rh + r;
        const bool ok = oc < B.OW && orow < B.OH;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(__builtin_fmaf(acc[r][e], dsc2, b2v[e]), 0.f);
        if (ok) amax = fmaxf(amax, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
        const unsigned o = ok ? 4u * (unsigned)(((n * B.OH + orow) * B.OW + oc) * 32 + nf2 * 16 + 4 * kq) : 0x80000000u;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u_t, v), yr, (int)o, 0, 0);
      }
    }
  }
  if (B.y_amax) amax_commit(B.y_amax, amax, blockIdx.x + wave, amax_peek(B.y_amax, blockIdx.x + wave));
  if (dead && lane == 0) atomicAdd(&g_pair_timeouts, 1u);
}

}  // namespace

// -1: not this kernel's problem.  force: skip the efficiency terms of the rule (tests).
int espcn_pair_launch(int N, int H, int W, const float* x, const void* w1p, const float* b1, const void* wp2,
                      const float* b2, float* y, float* x_amax, int amax_mode, float* y_amax, bool force, hipStream_t s) {
  if (N < 1 || H < 7 || W < 7 || !x_amax) return -1;
  const int OH = H - 6, OW = W - 6;
  const int tiles_y = (OH + PR_TH - 1) / PR_TH, tiles_x = (OW + PR_TW - 1) / PR_TW;
  const long ntiles = (long)N * tiles_y * tiles_x;
  const size_t x_img = (size_t)3 * H * W * 4, y_bytes = (size_t)N * OH * OW * 32 * 4;
  if (ntiles >= (1L << 29) || x_img >= (1ull << 31) || y_bytes >= (1ull << 31)) return -1;
  if (!force) {  // full-enough tiles, four tiles per CU
    if ((double)OH * OW < 0.85 * (double)tiles_y * tiles_x * (PR_TH * PR_TW)) return -1;
    if (ntiles < 4L * kNumCU) return -1;
  }
  // the fp16 section of the 64 -> 32 3x3 filter as conv_bfw_gather finds it
  const size_t elems = (size_t)9 * 64 * 32;
  const char* prepared = reinterpret_cast<const char*>(wp2) + bf3_prepared_offset(elems);
  const char* fsec = prepared + f16_section_offset(64, 32, 9);
  PairParams B{};
  B.x = x; B.w1p = reinterpret_cast<const uint4*>(w1p); B.b1 = b1; B.b2 = b2; B.y = y; B.x_amax = x_amax; B.y_amax = y_amax;
  B.xn = (size_t)N * 3 * H * W;
  B.amax_mode = amax_mode;
  B.wq2 = reinterpret_cast<const uint4*>(fsec);
  B.w2_descale = reinterpret_cast<const float*>(fsec + bf3_main_bytes(64, 32, 9));
  B.N = N; B.H = H; B.W = W; B.OH = OH; B.OW = OW; B.tiles_x = tiles_x; B.tiles_y = tiles_y; B.img_tiles = tiles_x * tiles_y;
  B.ntiles = (int)ntiles;
  B.x_img_bytes = (unsigned)x_img;
  B.y_bytes = (unsigned)y_bytes;
  int grid = kNumCU;
  if (grid > ntiles) grid = (int)ntiles;
  note_amax_written(y_amax != nullptr);
  note_kernel("k_espcn_pair");
  launch_lds<&k_espcn_pair>(dim3(grid), dim3(512), PR_LDS, s, B);
  return check_launch("espcn_pair");
}

int pair_ring_timeouts(int reset) {  // (srk_ring_timeouts, conv_bfr.hip)
  unsigned v = 0;
  if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_pair_timeouts), sizeof(v)) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  if (reset && v) {
    const unsigned z = 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_pair_timeouts), &z, sizeof(z));
  }
  return (int)v;
}

int pair_scans(int reset) {
  unsigned v = 0;
  if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_pair_scans), sizeof(v)) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  if (reset && v) {
    const unsigned z = 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_pair_scans), &z, sizeof(z));
  }
  return (int)v;
}

int espcn_pair_prepare(const float* w1, const float* b1, void* out, hipStream_t s) {
  hipLaunchKernelGGL(k_espcn_pair_prep, dim3(1), dim3(128), 0, s, w1, b1, reinterpret_cast<uint4*>(out));
  return check_launch("espcn_pair_prepare");
}
size_t espcn_pair_prepared_bytes() { return PR_W1P_BYTES; }

}  // namespace srk

extern "C" size_t srk_espcn_pair_prepared_bytes(void) { return srk::espcn_pair_prepared_bytes(); }

extern "C" int srk_espcn_pair_prepare(const float* w1, const float* b1, void* w1_prepared, void* stream) {
  SRK_REQUIRE(w1 && b1 && w1_prepared, "espcn_pair_prepare: null pointer");
  SRK_REQUIRE((uintptr_t)w1_prepared % 16 == 0, "espcn_pair_prepare: w1_prepared must be 16-byte aligned");
  return srk::espcn_pair_prepare(w1, b1, w1_prepared, (hipStream_t)stream);
}

extern "C" int srk_espcn_pair_scans(int reset) { return srk::pair_scans(reset); }

extern "C" int srk_espcn_pair_forward(int N, int H, int W, const float* x, const void* w1_prepared, const float* b1,
                                      const float* w2_packed_fwd, const float* b2, float* y, float* x_amax,
                                      int x_amax_compute, float* y_amax, int force, void* stream) {
  if (!x || !w1_prepared || !b1 || !w2_packed_fwd || !b2 || !y || !x_amax) return SRK_ERR_UNSUPPORTED;
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)w1_prepared) % 16 != 0) return SRK_ERR_UNSUPPORTED;
  const int mode = x_amax_compute ? ((force & 2) ? 2 : 1) : 0;
  const int rc = srk::espcn_pair_launch(N, H, W, x, w1_prepared, b1, w2_packed_fwd, b2, y, x_amax, mode, y_amax,
                                        (force & 1) != 0, (hipStream_t)stream);
  return rc == -1 ? SRK_ERR_UNSUPPORTED : rc;
}
