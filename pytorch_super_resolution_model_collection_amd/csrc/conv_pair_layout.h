// The staged input tile of k_espcn_pair (conv_pair.hip) and where a lane reads its first-layer pixel fragments in it: the
// one copy of that addressing, shared by the kernel and by tools/pair_lds_host_check.cpp, which counts the LDS bank
// conflicts of every (fragment, K step) on the CPU.  Plain constexpr C++: no device types.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRK_PR_HD __host__ __device__ __forceinline__ constexpr
#else
#define SRK_PR_HD inline constexpr
#endif

namespace srk {

constexpr int PR_HW = 18;                           // halo width of the second layer's tile (10 x 18)
constexpr int PR_NKEEP = 2 * PR_HW;                 // halo rows 0 .. 1 / 8 .. 9: pixels
constexpr int PR_XR = 14, PR_XC = 23, PR_XP = 24;   // staged input tile: rows, columns, cell pitch of a row (PQ and T)
constexpr int PR_XPQ = PR_XR * PR_XP * 16;          // bytes of a group's PQ [row][pixel]: 16-byte cells
constexpr int PR_XT = PR_XPQ + 32;                  // T [row][pixel] of 8-byte cells starts here (cells -3 .. -1 exist: staging)
constexpr int PR_XBUF = PR_XT + PR_XR * PR_XP * 8;  // bytes of a group's input tile
constexpr unsigned long long PR_FPIX = 0xfdb9eca875316420ull;   // nibble j: the fragment pixel of lane column j

// The first layer's K: 8 steps of 32, lane quarter kq supplies K values 8 kq .. 8 kq + 7 of step ks -- one K group.
//   PR_KTAP  tap (dy, dx): pixel side the PQ cell {h0 h1 h2 m0 m1 m2 h0 h1} of pixel (row + dy, col + dx), filter side
//            {wh0 wh1 wh2 wh0 wh1 wh2 wm0 wm1}: eight of the tap's nine products w_h x_h + w_h x_m + w_m x_h
//   PR_KROW  kernel row dy: pixel side T(row + dy, col), T(row + dy, col + 4) = h2 of eight pixels in a row, filter side
//            {wm2 of dx = 0 .. 4, 0, 0, 0}: the ninth product of the row's five taps
//   PR_KNONE zero weights against any staged cell
// Steps 0 .. 4: tap (ks, kq).  Step 5: tap (r, 4), r = 0, 2, 1, 3 for kq = 0 .. 3.  Step 6: tap (4, 4), none, rows 0, 2.
// Step 7: rows 1, 3, 4, none.  A lane's cell of steps 0 .. 4 is its own cell of step 0 plus ks rows: one base and an
// immediate.  Which groups share a step, and a lane pair (kq, kq + 1) inside it, is chosen for the LDS banks.
enum { PR_KTAP, PR_KROW, PR_KNONE };
struct PrKGroup {
  int kind, dy, dx;
};
SRK_PR_HD PrKGroup pr_kgroup(int ks, int kq) {
  if (ks < 5) return {PR_KTAP, ks, kq};
  if (ks == 5) return {PR_KTAP, (kq >> 1) + 2 * (kq & 1), 4};
  if (ks == 6) return kq == 0 ? PrKGroup{PR_KTAP, 4, 4} : (kq == 1 ? PrKGroup{PR_KNONE, 0, 0} : PrKGroup{PR_KROW, 2 * kq - 4, 0});
  return kq == 3 ? PrKGroup{PR_KNONE, 0, 0} : PrKGroup{PR_KROW, kq == 2 ? 4 : 2 * kq + 1, 0};
}

// Lane column j holds pixel PR_FPIX(j) of its 16-pixel fragment (which pixels share a 16-lane group of ds_read_b128).
SRK_PR_HD int pr_fpix(int j) { return (int)((PR_FPIX >> (4 * j)) & 15); }
// Pixel of the 10 x 18 halo that lane column j computes in fragment m of its wave: rows 2 .. 9 are nine fragments, the
// wave of pixel half mh takes f = 4 mh + m, m < 4, and the ninth as m = 4; rows 0 .. 1 are three, f = 2 mh + m, m < 2,
// clamped to the last pixel of row 1.
SRK_PR_HD int pr_body_pix(int mh, int m, int j) { return PR_NKEEP + 16 * (m < 4 ? 4 * mh + m : 8) + pr_fpix(j); }
SRK_PR_HD int pr_top_pix(int mh, int m, int j) {
  const int p = 16 * (2 * mh + m) + pr_fpix(j);
  return p < PR_NKEEP ? p : PR_NKEEP - 1;
}
// Offset in staged cells of halo pixel p for lane quarter kq: the pixel's cell kq columns on (xp: cell pitch of a row).
SRK_PR_HD int pr_cell_off(int p, int kq, int xp = PR_XP) { return (p / PR_HW) * xp + p % PR_HW + kq; }
// K steps 0 .. 4 read the PQ cell off + ks xp, step 5 off + pr_k5.
SRK_PR_HD int pr_k5(int kq, int xp = PR_XP) { return pr_kgroup(5, kq).dy * xp + 4 - kq; }
// Step 6 + s reads two 8-byte halves, at byte off * kmul + kadd and kd on: of the PQ cell of tap (4, 4) or of T's cells of
// the lane's row.  A lane without a K group reads what its neighbour reads (the same addresses cost no LDS cycle).
struct PrK67 {
  int kmul, kadd, kd;
};
SRK_PR_HD PrK67 pr_k67(int s, int kq, int xp = PR_XP, int xt = PR_XT) {
  const PrKGroup own = pr_kgroup(6 + s, kq), g = own.kind == PR_KNONE ? pr_kgroup(6 + s, kq - 1) : own;
  return g.kind == PR_KTAP ? PrK67{16, 16 * (g.dy * xp + g.dx - kq), 8} : PrK67{8, xt + 8 * (g.dy * xp - kq), 32};
}
// Byte address inside the group's staged tile of the read (K step ks, half h: 0, or 1 for the second 8 bytes of steps 6, 7)
SRK_PR_HD int pr_l1_addr(int off, int ks, int kq, int h, int xp = PR_XP, int xt = PR_XT) {
  if (ks < 6) return 16 * (off + (ks < 5 ? ks * xp : pr_k5(kq, xp)));
  const PrK67 k = pr_k67(ks - 6, kq, xp, xt);
  return off * k.kmul + k.kadd + h * k.kd;
}

}  // namespace srk
