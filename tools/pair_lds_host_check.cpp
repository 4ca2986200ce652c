// LDS bank conflicts of k_espcn_pair's first-layer fragment reads, counted on the CPU from the kernel's own addressing
// (csrc/conv_pair_layout.h, which conv_pair.hip includes too).  No device, no Python.  Build and run from the repo root:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/pair_lds_host_check.cpp -o pair_lds_host_check
//   ./pair_lds_host_check            the layout as built: a table per K step, one summary line
//   ./pair_lds_host_check --search   the same totals for every row pitch and T placement that fits the LDS
// For every fragment a wave computes (nine of halo rows 2 .. 9, three of rows 0 .. 1) and every K step it enumerates the
// byte address of each of the 64 lanes and applies the bank rule of the part: a wave's access is served in fixed lane
// groups, one LDS cycle per group; the bank of byte a is (a / 4) mod 64; lanes of a group that read the same dword
// share it, and every further distinct dword on a busy bank costs the group one more cycle.
//   ds_read_b128 (steps 0 .. 5): four groups of 16 lanes {0-3,12-15,20-27} {4-11,16-19,28-31} and the same + 32
//   ds_read_b64  (steps 6, 7: two per step): two groups of 32 lanes
// It also checks that every read is aligned to its width and lies inside the group's staged tile.
#include <stdio.h>
#include <string.h>

#include <map>
#include <set>

#include "../pytorch_super_resolution_model_collection_amd/csrc/conv_pair_layout.h"

using namespace srk;

static int g_bad = 0;   // misaligned or out-of-range reads

// extra LDS cycles of one wave instruction: lanes' byte addresses, `bytes` per lane
static int extra_cycles(const int* addr, int bytes) {
  int extra = 0;
  const int ngroups = bytes == 16 ? 4 : 2;
  for (int g = 0; g < ngroups; ++g) {
    std::map<int, std::set<int>> bank;   // bank -> distinct dwords
    for (int lane = 0; lane < 64; ++lane) {
      bool in;
      if (bytes == 16) {
        const int l = lane & 31, first = (l < 4) || (l >= 12 && l < 16) || (l >= 20 && l < 28);
        in = (lane >> 5) == (g >> 1) && (first ? 0 : 1) == (g & 1);
      } else {
        in = (lane >> 5) == g;
      }
      if (!in) continue;
      for (int d = 0; d < bytes / 4; ++d) bank[(addr[lane] / 4 + d) % 64].insert(addr[lane] / 4 + d);
    }
    size_t worst = 1;
    for (auto& b : bank) worst = b.second.size() > worst ? b.second.size() : worst;
    extra += (int)worst - 1;
  }
  return extra;
}

// extra cycles per K step (0 .. 7) over a wave's fragment of halo pixels pix(j), summed into out[]; reads counted in rd[]
template <class Pix>
static void fragment(Pix pix, int xp, int xt, int xbuf, int* out, int* rd) {
  for (int ks = 0; ks < 8; ++ks)
    for (int h = 0; h < (ks < 6 ? 1 : 2); ++h) {
      int addr[64];
      const int bytes = ks < 6 ? 16 : 8;
      for (int lane = 0; lane < 64; ++lane) {
        const int j = lane & 15, kq = lane >> 4;
        addr[lane] = pr_l1_addr(pr_cell_off(pix(j), kq, xp), ks, kq, h, xp, xt);
        if (addr[lane] % bytes || addr[lane] < 0 || addr[lane] + bytes > xbuf) ++g_bad;
      }
      out[ks] += extra_cycles(addr, bytes);
      rd[ks] += bytes == 16 ? 4 : 2;
    }
}

struct Totals {
  int body[8], top[8], rbody[8], rtop[8];
};

static Totals count(int xp, int xt) {
  Totals t;
  memset(&t, 0, sizeof(t));
  const int xbuf = xt + PR_XR * xp * 8;
  for (int mh = 0; mh < 2; ++mh) {
    for (int m = 0; m < (mh == 0 ? 5 : 4); ++m)   // fragment 8 (m = 4) once
      fragment([&](int j) { return pr_body_pix(mh, m, j); }, xp, xt, xbuf, t.body, t.rbody);
    for (int m = 0; m < 2; ++m)
      if (2 * mh + m < 3) fragment([&](int j) { return pr_top_pix(mh, m, j); }, xp, xt, xbuf, t.top, t.rtop);
  }
  return t;
}

int main(int argc, char** argv) {
  const bool search = argc > 1 && !strcmp(argv[1], "--search");
  if (!search) {
    const Totals t = count(PR_XP, PR_XT);
    printf("k_espcn_pair first-layer fragment reads, pitch %d cells, T at byte %d; LDS cycles per tile and channel chunk\n", PR_XP,
           PR_XT);
    printf("step  rows 2..9 (nine fragments): reads extra   rows 0..1 (three fragments): reads extra\n");
    int eb = 0, et = 0, e05 = 0, e67 = 0;
    for (int ks = 0; ks < 8; ++ks) {
      printf("%4d  %36d %5d %38d %5d\n", ks, t.rbody[ks], t.body[ks], t.rtop[ks], t.top[ks]);
      eb += t.body[ks];
      et += t.top[ks];
      (ks < 6 ? e05 : e67) += t.body[ks] + t.top[ks];
    }
    printf("pair_lds_host_check: pitch %d xt %d extra cycles steps 0-4 %d, step 5 %d, steps 6-7 %d (rows 2..9: %d, rows 0..1: %d), bad reads %d\n",
           PR_XP, PR_XT, e05 - t.body[5] - t.top[5], t.body[5] + t.top[5], e67, eb, et, g_bad);
    return g_bad ? 1 : 0;
  }
  // every pitch and T placement (in 8-byte steps over one bank period) whose two staged tiles fit the LDS left over
  const int spare = 2432;
  for (int xp = PR_XC + 1; xp <= 40; ++xp) {
    int best = -1, best_xt = 0, best5 = 0, best67 = 0;
    for (int gap = 32; gap < 32 + 256; gap += 8) {
      const int xt = PR_XR * xp * 16 + gap;
      if (2 * (xt + PR_XR * xp * 8) - 2 * PR_XBUF > spare) break;
      const Totals t = count(xp, xt);
      int e = 0, e67 = 0;
      for (int ks = 0; ks < 8; ++ks) e += t.body[ks], e67 += ks >= 6 ? t.body[ks] : 0;
      if (best < 0 || e < best) best = e, best_xt = xt, best5 = t.body[5], best67 = e67;
    }
    if (best < 0) {
      const Totals t = count(xp, PR_XR * xp * 16 + 32);
      int e = 0, e67 = 0;
      for (int ks = 0; ks < 8; ++ks) e += t.body[ks], e67 += ks >= 6 ? t.body[ks] : 0;
      printf("pitch %2d does not fit (needs %d bytes more than the %d spare): extra %d (step 5: %d, steps 6-7: %d)\n", xp,
             2 * (PR_XR * xp * 24 + 32) - 2 * PR_XBUF, spare, e, t.body[5], e67);
    } else {
      printf("pitch %2d fits: least extra over rows 2..9 %d (step 5: %d, steps 6-7: %d) with T at byte %d\n", xp, best, best5,
             best67, best_xt);
    }
  }
  return g_bad ? 1 : 0;
}
