"""TEST INFRASTRUCTURE: the case table of the weight-gradient branch tests, and the library's own answer for a row.

The host planner of csrc/conv_wgrad_bf16.hip lives in csrc/conv_wgrad_plan.h (wb_launch_plan: tile shape, split-K count,
tile / spec, prefetch, ring, k_wgrad_tr eligibility, grid, LDS, workspace, name).  `plan()` asks it through
srk_conv2d_backward_weight_plan -- a host-only call that needs no GPU -- "which kernel will srk_last_kernel_name() report
for this problem, and with which grid", so that tests/test_wgrad_plan_cpu.py keeps the table below on the branches its rows
name when the planner moves, and tests/test_wgrad_bf_gpu.py can assert the name on the device.

CASES is the table: one row per (kernel configuration, variant, K loop, staging mode, load width, dY layout, launch kind)
the planner can choose.  N is the smallest batch at which the row's variant is planned on 256 CUs."""
import collections
import ctypes

_FIELDS = ("name kernel cfg spec prefetch ring scalar grouped TH TW TWo HH tiles_y tiles_x ntiles G gy gz grid_x lds_bytes "
           "lds ring_bytes ws_bytes")
Plan = collections.namedtuple("Plan", _FIELDS + " swizzle idle_blocks")


def cdiv(a, b):
    return (a + b - 1) // b


def out_dims(H, W, KH, KW, pad):
    return H + 2 * pad - KH + 1, W + 2 * pad - KW + 1


def plan(N, H, W, Cin, Cout, KH, KW, pad, dy_ps_r=0, n=1, x_aligned=True, dy_aligned=True, num_cu=256):
    """-> Plan, or None where the planner refuses the problem.  dy_aligned covers dY and the mask (vec_y needs both)."""
    from pytorch_super_resolution_model_collection_amd import _lib as L
    OH, OW = out_dims(H, W, KH, KW, pad)
    d = L.ConvDesc(N, H, W, Cin, OH, OW, Cout, KH, KW, 1, pad, 0, 0, 0, 0, dy_ps_r)
    out = L.WgradPlan()
    L.check(L.load().srk_conv2d_backward_weight_plan(ctypes.byref(d), n, int(x_aligned), int(dy_aligned), num_cu,
                                                     ctypes.byref(out)), "srk_conv2d_backward_weight_plan")
    if not out.ok:
        return None
    f = {k: getattr(out, k) for k in _FIELDS.split() if k not in ("name", "kernel", "lds")}
    f.update(name=out.name.decode(), kernel=("bf", "tr")[out.kernel], lds=out.lds_set)
    for k in ("spec", "prefetch", "ring", "scalar", "grouped"):
        f[k] = bool(f[k])
    # two facts of the kernels' block -> tile mapping, not of the planner:
    swizzle = out.gy == 2 and out.grid_x % 8 == 0          # conv_wgrad_bf16.hip:232 (k_wgrad_bf), :863 (k_wgrad_tr)
    # ring / tr blocks take ceil(ntiles / G) consecutive tiles each (conv_wgrad_bf16.hip:729, :898): the last may get none
    idle = out.G - cdiv(out.ntiles, cdiv(out.ntiles, out.G)) if out.ring or out.kernel else 0
    return Plan(swizzle=swizzle, idle_blocks=idle * n, **f)


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
    """the library's plan of row c"""
    return plan(c.N, c.H, c.W, c.cin, c.cout, c.kh, c.kw, c.pad, dy_ps_r=c.ps, n=c.n, x_aligned=c.off[0] % 16 == 0,
                dy_aligned=c.off[1] % 16 == 0 and (c.mask is None or c.off[2] % 16 == 0), num_cu=num_cu)


def layer_mask(c, layer):
    return c.mask[layer] if isinstance(c.mask, tuple) else c.mask
