"""TEST INFRASTRUCTURE: the host planner of csrc/conv_wgrad_bf16.hip in plain Python, and the case table of the
weight-gradient branch tests.

`plan()` mirrors wb_plan (tile shape), wb_split (split-K count, tile / spec), wb_prefetch_ok, wb_ring_setup and wt_setup
(k_wgrad_tr eligibility) -- host integer / double arithmetic only, written from the planner's rules; it never calls the
library.  It answers "which kernel must srk_last_kernel_name() report for this problem, and with which grid", so that
tests/test_wgrad_plan_cpu.py can keep the table below on the branches its rows name when the planner's constants move,
and tests/test_wgrad_bf_gpu.py can assert the name on the device.

CASES is the table: one row per (kernel configuration, variant, K loop, staging mode, load width, dY layout, launch kind)
the planner can choose.  N is the smallest batch at which the row's variant is planned on 256 CUs."""
import collections

LDS_BUDGET = 74 * 1024     # kWbLdsBudget
MAXOCT = 64                # WB_MAXOCT
SST = 512                  # WB_SST
PIT = 1024 // SST          # WB_PIT
MAXGROUP = 40              # WB_MAXGROUP
CFG = {0: (32, 64, "2,2,2"), 1: (64, 32, "4,1,2"), 2: (64, 16, "4,1,1")}     # cfg -> CIB, COB, <CIT,COW,NTW>

Plan = collections.namedtuple(
    "Plan", "name kernel cfg spec prefetch ring scalar grouped TH TW TWo HH tiles_y tiles_x ntiles G gy gz swizzle "
            "idle_blocks lds ring_bytes")


def cdiv(a, b):
    return (a + b - 1) // b


def round_8odd(v):
    q = (v + 7) // 8
    if q % 2 == 0:
        q += 1
    return q * 8


def out_dims(H, W, KH, KW, pad):
    return H + 2 * pad - KH + 1, W + 2 * pad - KW + 1


def cfg_of(Cout):
    return 0 if Cout > 32 else (1 if Cout > 16 else 2)


def tile_candidates(cfg, KH, OH, OW):
    """(TWo, TH, lds) of every width wb_plan looks at: per width the tallest tile that fits (it stops there)"""
    CIB, COB, _ = CFG[cfg]
    TWo = 1
    while TWo <= 6 and (TWo - 1) * 8 < OW:
        TW = TWo * 8
        TH = min(16 // TWo, OH)
        while TH >= 1:
            HH, HWp = TH + KH - 1, TW + 8
            CS, DS = round_8odd(HH * HWp), round_8odd(TH * TW + 8)
            lds = (2 * CIB * CS + 2 * COB * DS) * 2
            if lds <= LDS_BUDGET and TH * TWo <= MAXOCT:
                yield TWo, TH, lds
                break
            TH -= 1
        TWo += 1


def prefetch_ok(cfg, TH, TW, KH, KW, H, W, Cin, OH, OW, Cout):
    CIB, COB, _ = CFG[cfg]
    HH = TH + KH - 1
    x_items = HH * ((TW + KW) >> 1) * (CIB // 4)
    y_items = TH * (TW >> 1) * (COB // 4)
    return (x_items <= PIT * SST and y_items <= PIT * SST and H * W * Cin * 4 < 2 ** 31 and OH * OW * Cout * 4 < 2 ** 31)


def ring_bytes(cfg, TH, TW, KH):
    """LDS of the ring mode (X ring of 2 HH rows + two dY buffer sets), 0 where it does not fit beside 8 KB of static LDS"""
    CIB, COB, _ = CFG[cfg]
    HH, HWp = TH + KH - 1, TW + 8
    b = (2 * CIB * round_8odd(2 * HH * HWp) + 2 * 2 * COB * round_8odd(TH * TW + 8)) * 2
    return b if b + 8 * 1024 <= 160 * 1024 else 0


def plan(N, H, W, Cin, Cout, KH, KW, pad, dy_ps_r=0, n=1, x_aligned=True, dy_aligned=True, num_cu=256, wgrad_tr=True):
    """-> Plan, or None where wb_plan refuses the problem.  dy_aligned covers dY and the mask (vec_y needs both)."""
    OH, OW = out_dims(H, W, KH, KW, pad)
    if KH > 3 or KW > 3 or Cin < 8 or Cout < 1:
        return None
    if H * W * Cin >= 2 ** 30 or OH * OW * Cout >= 2 ** 30:
        return None
    if dy_ps_r > 1 and (Cout % (dy_ps_r ** 2) != 0 or (Cout // dy_ps_r ** 2) % 4 != 0):
        return None
    if n > 1 and (dy_ps_r > 1 or n > MAXGROUP):
        return None
    cfg = cfg_of(Cout)
    CIB, COB, targs = CFG[cfg]
    best_eff, TH, TWo, lds = -1.0, 0, 0, 0
    for tTWo, tTH, tlds in tile_candidates(cfg, KH, OH, OW):
        tTW = tTWo * 8
        HH = tTH + KH - 1
        nks = cdiv(tTH * tTWo, 4)
        tiles = float(cdiv(OH, tTH) * cdiv(OW, tTW))
        cost = tiles * (nks + (float(HH) * (tTW + KW - 1) * CIB + float(tTH) * tTW * COB) / 3136.0)
        eff = float(OH) * OW / cost
        if eff > best_eff * 1.02 or (eff > best_eff * 0.98 and eff > 0 and tTH > TH):
            if eff > best_eff:
                best_eff = eff
            TH, TWo, lds = tTH, tTWo, tlds
    if best_eff < 0:
        return None
    TW, HH = TWo * 8, TH + KH - 1
    tiles_y, tiles_x = cdiv(OH, TH), cdiv(OW, TW)
    ntiles = N * tiles_y * tiles_x
    if ntiles > 2 ** 30:
        return None
    gy, gz = cdiv(Cin, CIB), cdiv(Cout, COB)
    # wb_split
    per = n * gy * gz
    g1, g2 = max(num_cu // per, 1), min(max(2 * num_cu // per, 1), ntiles)
    spec = 2 * lds + 8 * 1024 <= 160 * 1024 and ntiles >= 2 * g1
    G = g1 if spec else g2
    vec_x = Cin % 4 == 0 and x_aligned
    vec_y = Cout % 4 == 0 and dy_aligned
    prefetch = prefetch_ok(cfg, TH, TW, KH, KW, H, W, Cin, OH, OW, Cout) and vec_x and vec_y
    rb = ring_bytes(cfg, TH, TW, KH) if spec and prefetch else 0
    ring = rb > 0
    # wt_setup
    tr = spec and cfg == 0 and wgrad_tr and KH == 3 and KW == 3 and Cin % 32 == 0 and Cout % 64 == 0 and vec_x and vec_y
    if tr and dy_ps_r > 1 and (Cout // dy_ps_r ** 2) % 64 != 0:
        tr = False
    if tr and (H * W * Cin * 4 >= 2 ** 31 or OH * OW * Cout * 4 >= 2 ** 31):
        tr = False
    if tr and (HH * (TW + 2) * 4 > 1024 or TH * TW * 8 > 1024):
        tr = False
    if tr:
        XPL, YPL = 2 * HH * (TW + 4) * 64, (TH * TW + 8) * 128
        if 2 * XPL + 4 * YPL + 1024 > 160 * 1024 or 2 * XPL < SST * 9 * 4 or XPL + 512 >= 65536 or YPL + 1024 >= 65536:
            tr = False
    grouped = n > 1
    if tr:
        kernel, name = "tr", "k_wgrad_tr<%s>" % ("grouped" if grouped else "single")
    else:
        kernel = "bf"
        mode = "" if not spec else (",pf,ring" if prefetch and ring else (",pf" if prefetch else ""))
        name = "k_wgrad_bf<%s,%s%s%s%s>" % (targs, "spec" if spec else "tile", mode, "" if vec_x and vec_y else ",scalar",
                                            ",grouped" if grouped else "")
    idle = 0
    if ring or tr:     # a block takes ceil(ntiles / G) consecutive tiles: the last blocks may get none
        idle = G - cdiv(ntiles, cdiv(ntiles, G))
    swizzle = gy == 2 and (n * G) % 8 == 0
    return Plan(name, kernel, cfg, spec, bool(prefetch), ring, not (vec_x and vec_y), grouped, TH, TW, TWo, HH, tiles_y,
                tiles_x, ntiles, G, gy, gz, swizzle, idle * n, lds, rb)


# ---------------------------------------------------------------------------------------------------------------------
# The case table.  mask: None | "relu" | "lrelu" (grouped rows: every layer, or a tuple with one entry per layer);
# off = (x, dy, mask) byte offsets from a 16-byte boundary; want = facts of the plan the row was chosen for.
# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "row id n N cin cout kh kw pad H W mask ps off name want")


def _c(row, id, n, N, cin, cout, kh, kw, pad, H, W, name, mask=None, ps=0, off=(0, 0, 0), **want):
    return Case(row, id, n, N, cin, cout, kh, kw, pad, H, W, mask, ps, off, "k_wgrad_bf<%s>" % name, want)


CASES = [
    _c(1, "espcn2", 1, 86, 64, 32, 3, 3, 1, 24, 17, "4,1,2,spec", mask="relu", TH=12, prefetch=False),
    _c(2, "cout_tail", 1, 74, 64, 24, 3, 3, 1, 25, 20, "4,1,2,spec", TWo=3, prefetch=False),
    _c(3, "two_cin_chunks", 1, 37, 80, 32, 3, 3, 1, 25, 20, "4,1,2,spec", mask="lrelu", gy=2, swizzle=True),
    _c(4, "one_tile_row", 1, 103, 64, 32, 3, 3, 1, 8, 40, "4,1,2,spec,pf,ring", tiles_y=1, idle_blocks=84),
    _c(5, "fsrcnn_map", 1, 103, 12, 12, 3, 3, 1, 25, 20, "4,1,1,spec"),
    _c(6, "fsrcnn_map_nopad", 1, 256, 12, 12, 3, 3, 0, 18, 18, "4,1,1,spec"),
    _c(7, "fsrcnn_shrink", 1, 103, 56, 12, 1, 1, 0, 19, 29, "4,1,1,spec,pf,ring", mask="lrelu"),
    _c(8, "fsrcnn_expand", 1, 103, 12, 56, 1, 1, 0, 19, 29, "2,2,2,spec,pf,ring", mask="lrelu"),
    _c(9, "srcnn_1x1", 1, 47, 64, 32, 1, 1, 0, 33, 33, "4,1,2,spec,pf,ring", mask="relu", TWo=5, TH=3),
    _c(10, "espcn3", 1, 103, 32, 48, 3, 3, 1, 19, 29, "2,2,2,spec,pf,ring"),
    _c(11, "c48_64", 1, 52, 48, 64, 3, 3, 1, 19, 29, "2,2,2,spec,pf,ring", mask="relu", gy=2, swizzle=True, idle=True),
    _c(12, "c80_64", 1, 34, 80, 64, 3, 3, 1, 19, 29, "2,2,2,spec,pf,ring", gy=3, G=85),
    _c(13, "c32_80", 1, 52, 32, 80, 3, 3, 1, 19, 29, "2,2,2,spec,pf,ring", gz=2),
    _c(14, "c10_10", 1, 103, 10, 10, 3, 3, 1, 25, 20, "4,1,1,spec,scalar", mask="lrelu"),
    _c(15, "c10_12", 1, 103, 10, 12, 3, 3, 1, 25, 20, "4,1,1,spec,scalar"),
    _c(16, "c12_10", 1, 103, 12, 10, 3, 3, 1, 25, 20, "4,1,1,spec,scalar", mask="relu"),
    _c(17, "c9_33", 1, 103, 9, 33, 3, 3, 1, 19, 29, "2,2,2,spec,scalar"),
    _c(18, "x_unaligned", 1, 52, 64, 64, 3, 3, 1, 19, 29, "2,2,2,spec,scalar", off=(4, 0, 0)),
    _c(19, "dy_unaligned", 1, 86, 64, 32, 3, 3, 1, 19, 29, "4,1,2,spec,scalar", mask="relu", off=(0, 4, 4)),
    _c(20, "mask_unaligned", 1, 52, 64, 64, 3, 3, 1, 19, 29, "2,2,2,spec,scalar", mask="relu", off=(0, 0, 8)),
    _c(21, "ps2_C16", 1, 103, 32, 64, 3, 3, 1, 19, 29, "2,2,2,spec,pf,ring", ps=2),
    _c(22, "ps2_C8", 1, 74, 64, 32, 3, 3, 1, 25, 20, "4,1,2,spec", ps=2),
    _c(23, "ps2_C4", 1, 103, 16, 16, 3, 3, 1, 25, 20, "4,1,1,spec", ps=2),
    _c(24, "k2x2", 1, 103, 64, 32, 2, 2, 0, 25, 20, "4,1,2,spec", prefetch=False),
    _c(25, "k2x2_pad", 1, 86, 16, 8, 2, 2, 1, 25, 20, "4,1,1,spec", TH=14),
    _c(26, "k1x3", 1, 52, 40, 40, 1, 3, 0, 19, 29, "2,2,2,spec,pf,ring", gy=2),
    _c(27, "k3x1", 1, 103, 16, 12, 3, 1, 1, 25, 20, "4,1,1,spec"),
    _c(28, "grp_64_32", 3, 29, 64, 32, 3, 3, 1, 24, 17, "4,1,2,spec,grouped", mask=("relu", None, "relu")),
    _c(29, "grp_12_12", 4, 26, 12, 12, 3, 3, 1, 25, 20, "4,1,1,spec,grouped"),
    _c(30, "grp_1x1", 3, 34, 56, 12, 1, 1, 0, 19, 29, "4,1,1,spec,pf,ring,grouped", mask="lrelu"),
    _c(31, "grp_48_64", 2, 26, 48, 64, 3, 3, 1, 19, 29, "2,2,2,spec,pf,ring,grouped", swizzle=True, idle=True),
    _c(32, "grp_scalar", 3, 34, 10, 10, 3, 3, 1, 25, 20, "4,1,1,spec,scalar,grouped"),
    _c(33, "tile_swizzle", 1, 4, 64, 64, 3, 3, 1, 12, 16, "2,2,2,tile", G=8, gy=2, swizzle=True),
    _c(34, "tile_scalar", 1, 2, 10, 10, 3, 3, 1, 9, 11, "4,1,1,tile,scalar", mask="lrelu"),
    _c(35, "tile_unaligned", 1, 2, 64, 32, 3, 3, 1, 12, 12, "4,1,2,tile,scalar", off=(4, 4, 0)),
    _c(36, "tile_ps_C16", 1, 2, 32, 64, 3, 3, 1, 9, 11, "2,2,2,tile", ps=2),
]
BY_ID = {c.id: c for c in CASES}


def plan_case(c, num_cu=256):
    return plan(c.N, c.H, c.W, c.cin, c.cout, c.kh, c.kw, c.pad, dy_ps_r=c.ps, n=c.n, x_aligned=c.off[0] % 16 == 0,
                dy_aligned=c.off[1] % 16 == 0 and (c.mask is None or c.off[2] % 16 == 0), num_cu=num_cu)


def layer_mask(c, layer):
    return c.mask[layer] if isinstance(c.mask, tuple) else c.mask
