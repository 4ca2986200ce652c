// Host planner of the stride-1 bf16x3 weight gradient (conv_wgrad_bf16.hip: k_wgrad_bf, k_wgrad_tr): tile shape, split-K
// count, staging mode, kernel, grid, LDS, workspace and the name srk_last_kernel_name() reports -- one value,
// srk_wgrad_plan (include/srk.h), made by wb_launch_plan() and consumed by every launcher, workspace query and
// srk_conv2d_backward_weight_plan().  Plain C++17: no HIP runtime call, no device code, no environment switch -- the CU
// count and SRK_WGRAD_TR come in as arguments, so the tests ask this code for its decisions on any machine.
#pragma once
#include <stddef.h>
#include "../../include/srk.h"

namespace srk {

constexpr int WB_MAXOCT = 64;  // octets per tile (<= 512 pixels)
constexpr int WB_SST = 512;    // SPEC: staging threads (8 waves next to the 4 working waves; 4 stager waves: 0.157 -> 0.20 ms on the VDSR layer)
constexpr int WB_PIT = 1024 / WB_SST;  // SPEC stagers: register batches per tensor and tile when prefetching one tile ahead
constexpr int WB_MAXGROUP = 40;        // layers of one grouped launch (their pointers travel in the kernel arguments)
constexpr int kWbLdsBudget = 74 * 1024;  // + ~4.6 KB static (tables, bias reduction): 2 blocks per CU
constexpr int kWbLdsMax = 160 * 1024;    // LDS of a CU
constexpr int kWbLdsStatic = 8 * 1024;   // what a block's static LDS may take beside its dynamic LDS

// cfg 0: 32 ci x 64 co (CIT 2, COW 2, NTW 2); 1: 64 ci x 32 co (4,1,2); 2: 64 ci x 16 co (4,1,1)
struct WbCfg {
  int CIB, COB, CIT, COW, NTW;
  const char* targs;  // "CIT,COW,NTW" as the kernel's name spells it
};
constexpr WbCfg kWbCfg[3] = {{32, 64, 2, 2, 2, "2,2,2"}, {64, 32, 4, 1, 2, "4,1,2"}, {64, 16, 4, 1, 1, "4,1,1"}};

constexpr int wb_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

constexpr int round_8odd(int v) {  // smallest multiple of 8 >= v whose quotient by 8 is odd
  int q = (v + 7) / 8;
  if ((q & 1) == 0) ++q;
  return q * 8;
}

// LDS of one buffer set of a TH x TWo-octet tile: bf16 hi | lo planes of the X halo and of the dY tile
constexpr size_t wb_tile_lds(int cfg, int KH, int TH, int TWo) {
  const int CS = round_8odd((TH + KH - 1) * (TWo * 8 + 8)), DS = round_8odd(TH * TWo * 8 + 8);
  return ((size_t)2 * kWbCfg[cfg].CIB * CS + (size_t)2 * kWbCfg[cfg].COB * DS) * 2;
}
// Ring mode of the wave-specialised kernel (WgBfParams.ring): the LDS of the 2 * HH-row ring and two dY buffer sets; 0
// when that does not fit
constexpr size_t wb_ring_lds(int cfg, int KH, int TH, int TWo) {
  const int cs_ring = round_8odd(2 * (TH + KH - 1) * (TWo * 8 + 8)), DS = round_8odd(TH * TWo * 8 + 8);
  const size_t bytes = ((size_t)2 * kWbCfg[cfg].CIB * cs_ring + (size_t)2 * 2 * kWbCfg[cfg].COB * DS) * 2;
  return bytes + kWbLdsStatic <= (size_t)kWbLdsMax ? bytes : 0;
}
constexpr bool wb_tile_fits(int cfg, int KH, int TH, int TWo) {
  return wb_tile_lds(cfg, KH, TH, TWo) <= (size_t)kWbLdsBudget && TH * TWo <= WB_MAXOCT;
}

// for every tile wb_plan can choose -- any configuration, kernel height, width and height inside the LDS
// budget -- the ring fits and so do two buffer sets.  Hence `prefetch && !ring` cannot be planned (the kernel's non-ring
// prefetch path is dead) and wb_split's LDS clause never decides.
constexpr bool wb_every_tile_takes_the_ring() {
  for (int cfg = 0; cfg < 3; ++cfg)
    for (int KH = 1; KH <= 3; ++KH)
      for (int TWo = 1; TWo <= 6; ++TWo)
        for (int TH = 1; TH <= 16 / TWo; ++TH) {
          if (!wb_tile_fits(cfg, KH, TH, TWo)) continue;
          if (wb_ring_lds(cfg, KH, TH, TWo) == 0) return false;
          if (2 * wb_tile_lds(cfg, KH, TH, TWo) + kWbLdsStatic > (size_t)kWbLdsMax) return false;
        }
  return true;
}
static_assert(wb_every_tile_takes_the_ring(), "a plannable k_wgrad_bf tile without room for the ring or two buffer sets");

struct WbPlan {
  bool ok;
  int cfg, CIB, COB;
  int TH, TW, TWo, tiles_y, tiles_x, HH, HWp, CS, DS, nks;
  size_t lds;
  int ntiles, gy, gz;
};

constexpr WbPlan wb_plan(const srk_conv_desc& d) {
  WbPlan pl{};
  pl.ok = false;
  if (d.transposed || d.stride != 1 || d.KH > 3 || d.KW > 3 || d.Cin < 8 || d.Cout < 1) return pl;
  if ((long)d.H * d.W * d.Cin >= (1L << 30) || (long)d.OH * d.OW * d.Cout >= (1L << 30)) return pl;  // 32-bit in-image offsets
  if (d.dy_ps_r > 1 && (d.Cout % (d.dy_ps_r * d.dy_ps_r) != 0 || (d.Cout / (d.dy_ps_r * d.dy_ps_r)) % 4 != 0)) return pl;
  pl.cfg = d.Cout > 32 ? 0 : (d.Cout > 16 ? 1 : 2);
  pl.CIB = kWbCfg[pl.cfg].CIB;
  pl.COB = kWbCfg[pl.cfg].COB;
  // tile = TH rows x TWo octets (8 pixels each).  Search the shapes that fit LDS for the one with the most useful
  // pixels per padded K step (e.g. 41-wide VDSR patches: 2 x 48 -> 83 % instead of 4 x 32 -> 60 %); ties -> taller
  // tiles (less halo per pixel).
  double best_eff = -1.0;
  for (int TWo = 1; TWo <= 6 && (TWo - 1) * 8 < d.OW; ++TWo) {
    const int TW = TWo * 8;
    int TH = 16 / TWo;  // <= 128 pixels per tile
    if (TH > d.OH) TH = d.OH;
    for (; TH >= 1; --TH) {
      if (!wb_tile_fits(pl.cfg, d.KH, TH, TWo)) continue;
      const int HH = TH + d.KH - 1;
      const int nks = wb_cdiv(TH * TWo, 4);
      const double tiles = (double)wb_cdiv(d.OH, TH) * wb_cdiv(d.OW, TW);
      // cost per tile: nks K steps + staging, calibrated on the VDSR / EDSR body layers (ablation: staging one
      // channel-pixel costs 1/3136 of a K step; only TW + KW - 1 halo columns are loaded)
      const double cost = tiles * (nks + ((double)HH * (TW + d.KW - 1) * pl.CIB + (double)TH * TW * pl.COB) / 3136.0);
      const double eff = (double)d.OH * d.OW / cost;
      if (eff > best_eff * 1.02 || (eff > best_eff * 0.98 && eff > 0 && TH > pl.TH)) {
        if (eff > best_eff) best_eff = eff;
        pl.TWo = TWo; pl.TW = TW; pl.TH = TH;
      }
      break;  // smaller TH only gets worse for this width
    }
  }
  if (best_eff < 0) return pl;
  pl.HH = pl.TH + d.KH - 1;
  pl.HWp = pl.TW + 8;
  pl.CS = round_8odd(pl.HH * pl.HWp);
  pl.DS = round_8odd(pl.TH * pl.TW + 8);
  pl.lds = wb_tile_lds(pl.cfg, d.KH, pl.TH, pl.TWo);
  pl.tiles_x = wb_cdiv(d.OW, pl.TW);
  pl.tiles_y = wb_cdiv(d.OH, pl.TH);
  pl.nks = wb_cdiv(pl.TH * pl.TWo, 4);
  const long nt = (long)d.N * pl.tiles_y * pl.tiles_x;
  if (nt > (1L << 30)) return pl;
  pl.ntiles = (int)nt;
  pl.gy = wb_cdiv(d.Cin, pl.CIB);
  pl.gz = wb_cdiv(d.Cout, pl.COB);
  pl.ok = true;
  return pl;
}

// Split-K count G of a launch over n layers of this plan (the per-layer entry: n = 1) and whether the wave-specialised
// variant runs it: one block per CU with two LDS buffer sets when every block then has >= 2 tiles to pipeline, else two
// resident blocks per CU.  spec == nullptr: the larger of the two counts, which the workspace is sized for.
constexpr int wb_split(const WbPlan& pl, int n, int num_cu, bool* spec) {
  const int per = n * pl.gy * pl.gz;  // (layer, channel-chunk) pairs
  int g1 = num_cu / per, g2 = (2 * num_cu) / per;
  if (g1 < 1) g1 = 1;
  if (g2 < 1) g2 = 1;
  if (g2 > pl.ntiles) g2 = pl.ntiles;
  if (!spec) return g2;
  *spec = 2 * pl.lds + kWbLdsStatic <= (size_t)kWbLdsMax && pl.ntiles >= 2 * g1;
  return *spec ? g1 : g2;
}

// SPEC stagers prefetch one tile ahead when a tile's pixel pairs fit their register batches (WB_PIT x 512 items per tensor)
constexpr bool wb_prefetch_ok(const WbPlan& pl, const srk_conv_desc& d) {
  const long x_items = (long)pl.HH * ((pl.TW + d.KW) >> 1) * (pl.CIB / 4);
  const long y_items = (long)pl.TH * (pl.TW >> 1) * (pl.COB / 4);
  // the prefetching stagers load through per-image buffer descriptors with 32-bit byte offsets
  const long ximg = (long)d.H * d.W * d.Cin * 4, yimg = (long)d.OH * d.OW * d.Cout * 4;
  return x_items <= (long)WB_PIT * WB_SST && y_items <= (long)WB_PIT * WB_SST && ximg < (1L << 31) && yimg < (1L << 31);
}

// Ring mode: plane stride of the 2 * HH-row ring and the LDS it needs; 0 when it does not apply.
constexpr size_t wb_ring_setup(const WbPlan& pl, const srk_conv_desc& d, bool prefetch, int& cs_ring) {
  if (!prefetch) return 0;
  cs_ring = round_8odd(2 * pl.HH * pl.HWp);
  return wb_ring_lds(pl.cfg, d.KH, pl.TH, pl.TWo);
}

// k_wgrad_tr (pixel-major LDS image + transpose reads): eligibility and LDS layout (L.XP / XPL / YPL, the LDS bytes)
constexpr bool wt_setup(srk_wgrad_plan& L, const srk_conv_desc& d, const WbPlan& pl, bool wgrad_tr, size_t& lds_bytes) {
  if (!L.spec || pl.cfg != 0 || !wgrad_tr) return false;
  if (d.KH != 3 || d.KW != 3 || d.Cin % 32 != 0 || d.Cout % 64 != 0 || L.scalar) return false;
  if (d.dy_ps_r > 1 && (d.Cout / (d.dy_ps_r * d.dy_ps_r)) % 64 != 0) return false;
  const long ximg = (long)d.H * d.W * d.Cin * 4, yimg = (long)d.OH * d.OW * d.Cout * 4;
  if (ximg >= (1L << 31) || yimg >= (1L << 31)) return false;   // per-image buffer descriptors, 32-bit byte offsets
  if ((long)pl.HH * (pl.TW + 2) * 4 > 1024 || (long)pl.TH * pl.TW * 8 > 1024) return false;  // two items per stager and tensor
  const int XP = pl.TW + 4;   // halo columns 0 .. TW + 1 are staged; the third transpose read of a row touches TW + 3
  const size_t XPL = (size_t)2 * pl.HH * XP * 64, YPL = (size_t)(pl.TH * pl.TW + 8) * 128;
  const size_t bytes = 2 * XPL + 4 * YPL;
  if (bytes + 1024 > (size_t)kWbLdsMax || 2 * XPL < (size_t)WB_SST * 9 * 4 || XPL + 512 >= 65536 || YPL + 1024 >= 65536) return false;
  L.XP = XP;
  L.XPL = (int)XPL;
  L.YPL = (int)YPL;
  lds_bytes = bytes;
  return true;
}

// dst = the concatenation of parts (this runs on every dispatch: no printf)
template <size_t N, size_t M>
inline void wb_name(char (&dst)[N], const char* const (&parts)[M]) {
  size_t o = 0;
  for (const char* s : parts)
    for (; *s && o + 1 < N; ++s) dst[o++] = *s;
  dst[o] = 0;
}

// The whole decision for a launch over n layers of geometry d.  grouped: the grouped entry (its kernels take the layer from
// blockIdx.x; a chunk of one layer is still a grouped launch).  x_aligned / y_aligned: every x / every dY and mask pointer
// is on a 16-byte boundary.  bias_ws: what the per-layer entry keeps behind its slabs for the bias-gradient finish.
inline srk_wgrad_plan wb_launch_plan(const srk_conv_desc& d, int n, bool grouped, bool x_aligned, bool y_aligned, int num_cu,
                                     bool wgrad_tr, size_t bias_ws) {
  srk_wgrad_plan L{};
  L.struct_size = (uint32_t)sizeof(L);
  const WbPlan pl = wb_plan(d);
  if (!pl.ok || n < 1 || num_cu < 1 || (grouped && (n > WB_MAXGROUP || d.dy_ps_r > 1)) || (!grouped && n != 1)) return L;
  const WbCfg& c = kWbCfg[pl.cfg];
  bool spec = false;
  L.G = wb_split(pl, n, num_cu, &spec);
  L.n = n;
  L.grouped = grouped;
  L.cfg = pl.cfg; L.CIB = pl.CIB; L.COB = pl.COB;
  L.spec = spec;
  L.k33 = spec && d.KH == 3 && d.KW == 3;
  L.vec_x = d.Cin % 4 == 0 && x_aligned;
  L.vec_y = d.Cout % 4 == 0 && y_aligned;
  L.scalar = !(L.vec_x && L.vec_y);
  L.prefetch = spec && wb_prefetch_ok(pl, d) && !L.scalar;  // the spec stagers' mode (no other variant reads it); 16-byte channel groups only
  L.TH = pl.TH; L.TW = pl.TW; L.TWo = pl.TWo; L.HH = pl.HH; L.HWp = pl.HWp; L.CS = pl.CS; L.DS = pl.DS; L.nks = pl.nks;
  L.tiles_y = pl.tiles_y; L.tiles_x = pl.tiles_x; L.ntiles = pl.ntiles; L.gy = pl.gy; L.gz = pl.gz;
  L.lds_set = (int32_t)pl.lds;
  int cs_ring = 0;
  if (const size_t ring_bytes = wb_ring_setup(pl, d, L.prefetch, cs_ring)) {
    L.ring = 1;
    L.ring_bytes = (int32_t)ring_bytes;
    L.CS = cs_ring;  // the plane stride of the ring
  }
  L.grid_x = n * L.G; L.grid_y = pl.gy; L.grid_z = pl.gz;
  size_t lds = spec ? (L.ring ? (size_t)L.ring_bytes : 2 * pl.lds) : pl.lds;
  L.block = 64 * c.CIT * c.COW + (spec ? WB_SST : 0);
  if (wt_setup(L, d, pl, wgrad_tr, lds)) {
    L.kernel = SRK_WGRAD_KERNEL_TR;
    const char* const parts[] = {"k_wgrad_tr<", grouped ? "grouped" : "single", ">"};
    wb_name(L.name, parts);
  } else {
    // variant word, then what the shape and the pointers decided: the stagers' mode (spec only), the scalar loads, the group
    L.kernel = SRK_WGRAD_KERNEL_BF;
    const char* const parts[] = {"k_wgrad_bf<", c.targs, spec ? ",spec" : ",tile", !L.prefetch ? "" : (L.ring ? ",pf,ring" : ",pf"),
                                 L.scalar ? ",scalar" : "", grouped ? ",grouped" : "", ">"};
    wb_name(L.name, parts);
  }
  L.lds_bytes = (int32_t)lds;
  // workspace: split-K partial slabs [G][taps][Cin][Cout], then the bias partials.  The per-layer entry lays it out for the
  // larger of the two split counts, whichever variant runs; the grouped one for the count it launches, and asks for the larger.
  const size_t elems = (size_t)d.KH * d.KW * d.Cin * d.Cout;
  const size_t g2 = (size_t)wb_split(pl, n, num_cu, nullptr);
  if (grouped) {
    L.slab_bytes = (size_t)n * L.G * elems * sizeof(float);
    L.ws_bytes = (size_t)n * g2 * (elems + d.Cout) * sizeof(float);
  } else {
    L.slab_bytes = g2 * elems * sizeof(float);
    L.ws_bytes = L.slab_bytes + bias_ws;
  }
  L.ok = 1;
  return L;
}

}  // namespace srk
