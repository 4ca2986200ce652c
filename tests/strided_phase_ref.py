"""TEST INFRASTRUCTURE: the library's phase decomposition of strided TRANS gathers (csrc/conv_tile.h: phase_axis,
for_each_trans_phase, which for_each_phase launches from), and the case table of the strided / transposed convolution tests.

A ConvTranspose2d forward and the data gradient of a strided Conv2d are "TRANS gathers": out[oy] = sum over kh of
in[(oy + p - kh) / s] * w[kh] where the division is exact.  The library splits one into s x s stride-1 problems, one per
output phase; `phases()` and `phases_1d()` ask it for them through srk_trans_phases / srk_trans_phase_axis, host-only calls
that need no GPU.  tests/test_strided_phase_cpu.py runs a transposed convolution phase by phase through them against torch
in float64, and checks every declared property of the table below against them; tests/test_strided_gpu.py runs the table
on the device.

CASES: one row per (kernel family, block configuration, arithmetic, epilogue, phase geometry).  A row's `props` are the
edges it is in the table for -- the CPU test recomputes them from the library's phases, so a row can neither claim an edge
it does not have nor have one it does not claim:
  zero_tap     a phase with no tap at all (kernel smaller than the stride): its outputs are the epilogue of zero
  skipped      fewer than s x s phases run (oy0 >= OH or ox0 >= OW)
  uneven_taps  the phases that have taps differ in their tap counts
  multi_tile   a phase (a CONV gather: the output) has more pixels than one block of the row's kernel covers (`block`)
  dead_rows    data gradient of a strided conv: trailing dx rows / columns that no dy reaches although their phase has taps
Shapes: spatial sizes 1 .. 40, N 1 .. 3, the smallest at which the row's kernel and edge still occur on 256 CUs."""
import collections


def _lib():
    from pytorch_super_resolution_model_collection_amd import _lib as L
    return L


def out_dim(n, k, stride, pad, transposed, out_pad):
    """srk_conv_out_dim"""
    return _lib().load().srk_conv_out_dim(n, k, stride, pad, int(transposed), out_pad)


Phase = collections.namedtuple("Phase", "oy0 ox0 PH PW KHv KWv iy0 ix0 wh0 wdh ww0 wdw")


def _query(fn, record, args, most):
    out = (record * most)()
    out[0].struct_size = record().struct_size
    n = fn(*(args + (out, most)))
    assert 0 <= n <= most, (n, _lib().load().srk_last_error_string())
    return out[:n]


def phases(KH, KW, stride, pad, OH, OW):
    """srk_trans_phases: this launch produces outputs (oy0 + r*st, ox0 + c*st), r < PH, c < PW; virtual tap (u, v) reads
    input (r + iy0 + u, c + ix0 + v) and weight tap (wh0 + wdh*u, ww0 + wdw*v)."""
    L = _lib()
    return [Phase(*(getattr(q, f) for f in Phase._fields))
            for q in _query(L.load().srk_trans_phases, L.Phase, (KH, KW, stride, pad, OH, OW), stride * stride)]


def phases_1d(K, stride, pad, O):
    """srk_trans_phase_axis, one axis of phases(): (o0, P, Kv, i0, w0, wd) per phase that runs"""
    L = _lib()
    return [(a.o0, a.P, a.Kv, a.i0, a.w0, a.wd)
            for a in _query(L.load().srk_trans_phase_axis, L.PhaseAxis, (K, stride, pad, O), stride)]


# ---- the GPU table ---------------------------------------------------------------------------------------------------
# kind: "fwd" srk_conv2d_forward, "dgrad" srk_conv2d_backward_data, "wgrad" srk_conv2d_backward_weight
# tr: srk_conv_desc.transposed;  (H, W, cin) describe x, (OH, OW, cout) y, as in the descriptor
# algo: auto | bf16x6 | f16x3 | mfma_fp32 | generic;  env: SRK_* switches set for the call
# epi: fwd  b bias, l LeakyReLU(0.2), P per-channel PReLU, r residual;  dgrad  m LeakyReLU(0.2) mask on dy, a add_to;
#      wgrad  m mask, n "also with db = NULL"
# off: bytes past a 16-byte boundary of (the gather's input, its output)
# prefix: what srk_last_kernel_name() must start with (per-phase launches: the last phase's kernel)
# block: pixels of one block of that kernel (multi_tile);  exact: "zero_tap" | "dead" bit-exact clause
# tol: the bar, by the arithmetic that runs: 1e-4 bf16x3 class (TOL_ALGO["auto"]), 2e-5 (TOL_TIGHT) for bf16x6, f16x3 and
#      the exact-fp32 kernels (k_conv_mfma*, k_conv_direct, k_gather_conv, k_wgrad_mfma; k_conv_tapn's single-group form is
#      the exact 3-way split in every class, its multi-group form bf16x3 under "auto")
Case = collections.namedtuple("Case", "id kind tr cin cout kh kw s p op N H W algo env epi off prefix block props exact tol")

TOL_BF, TOL_TIGHT = 1e-4, 2e-5
MP0 = (("SRK_BFD_MP", "0"),)
BIG = (("SRK_BFD_SMALL", "0"),)                                   # bf16x6 / f16x3: k_conv_bfd's large blocks
BIG3 = (("SRK_BFD_SMALL", "0"), ("SRK_BF3_DIRECT", "1"))          # bf16x3: the same (SRK_BFD_SMALL=0 alone: k_conv_bf3)
_MP = "k_conv_bfd_mp<1,1,4,2,2,"


def _c(id, kind, tr, ch, k, s, p, op, size, prefix, algo="auto", env=(), epi="", off=(0, 0), block=None, props="",
       exact=None, tol=None):
    kh, kw = k if isinstance(k, tuple) else (k, k)
    if tol is None:
        tol = TOL_BF if algo == "auto" else TOL_TIGHT
    return Case(id, kind, tr, ch[0], ch[1], kh, kw, s, p, op, size[0], size[1], size[2], algo, tuple(env), epi, off, prefix,
                block, frozenset(props.split()), exact, tol)


CASES = [
    # ---- ConvTranspose2d forward: all phases in one launch (stride 2, Cout >= 64, small block) ----
    _c("mp_lapsrn_feat", "fwd", 1, (64, 64), 4, 2, 1, 0, (1, 13, 9), _MP + "2>x4", epi="bl", block=64, props="multi_tile"),
    _c("mp_k3_op1", "fwd", 1, (64, 64), 3, 2, 1, 1, (2, 7, 5), _MP + "2>x4", epi="b", block=64, props="uneven_taps"),
    _c("mp_k5_res", "fwd", 1, (64, 64), 5, 2, 2, 1, (1, 6, 7), _MP + "2>x4", epi="r", block=64, props="uneven_taps"),
    _c("mp_ksplit_128", "fwd", 1, (128, 64), 4, 2, 1, 0, (1, 5, 6), _MP + "2>x4", epi="bl", block=64),
    _c("mp_no_ksplit", "fwd", 1, (32, 64), 3, 2, 1, 1, (3, 5, 7), _MP + "1>x4", epi="bl", block=64, props="uneven_taps"),
    _c("mp_k1_zero", "fwd", 1, (64, 64), 1, 2, 0, 1, (2, 6, 5), _MP + "2>x4", epi="blr", block=64, props="zero_tap",
       exact="zero_tap"),
    _c("mp_cout128", "fwd", 1, (64, 128), 4, 2, 1, 0, (1, 4, 5), _MP, epi="b", block=64),
    _c("mp_k3_x6", "fwd", 1, (64, 64), 3, 2, 1, 1, (2, 7, 5), "k_conv_bfd_mp<1,1,4,3,2,2>x4", algo="bf16x6", epi="bl",
       block=64, props="uneven_taps"),
    # ---- per-phase launches of the small block, NOW = 1 .. 4 channel waves ----
    _c("ph_now1_fsrcnn", "fwd", 1, (8, 8), 9, 4, 3, 1, (2, 11, 6), "k_conv_bfd<1,1,1,2,2,", env=MP0, epi="b", block=64,
       props="uneven_taps multi_tile"),
    _c("ph_now2_k8", "fwd", 1, (24, 24), 8, 4, 2, 0, (1, 6, 9), "k_conv_bfd<1,1,2,2,2,", env=MP0, epi="bl", block=64),
    _c("ph_now3_k2_zero", "fwd", 1, (56, 40), 2, 4, 0, 0, (2, 5, 4), "k_conv_bfd<1,1,3,2,2,", env=MP0, epi="blr", block=64,
       props="zero_tap", exact="zero_tap"),
    _c("ph_now4_k3_zero", "fwd", 1, (80, 64), 3, 4, 0, 0, (1, 4, 5), "k_conv_bfd<1,1,4,2,2,", env=MP0, epi="blr", block=64,
       props="zero_tap", exact="zero_tap"),
    _c("ph_1x1_input", "fwd", 1, (8, 24), 2, 4, 0, 0, (3, 1, 1), "k_conv_bfd<1,1,2,2,2,", env=MP0, epi="b", block=64,
       props="skipped"),
    _c("ph_1xW_input", "fwd", 1, (24, 8), 3, 2, 1, 0, (2, 1, 9), "k_conv_bfd<1,1,1,2,2,", env=MP0, epi="bl", block=64,
       props="skipped uneven_taps"),
    _c("ph_3x5", "fwd", 1, (56, 40), (3, 5), 2, 1, 0, (1, 7, 6), "k_conv_bfd<1,1,3,2,2,", env=MP0, epi="b", block=64,
       props="uneven_taps"),
    _c("ph_mp0_c64", "fwd", 1, (64, 64), 4, 2, 1, 0, (1, 13, 9), "k_conv_bfd<1,1,4,2,2,", env=MP0, epi="bl", block=64,
       props="multi_tile"),
    _c("ph_k5_s3", "fwd", 1, (24, 40), 5, 3, 2, 2, (1, 5, 7), "k_conv_bfd<1,1,3,2,2,", env=MP0, epi="lr", block=64,
       props="uneven_taps"),
    _c("ph_x_unaligned", "fwd", 1, (24, 24), 4, 2, 1, 0, (1, 6, 5), "k_conv_bfd<1,1,2,2,2,", env=MP0, epi="b", off=(4, 0),
       block=64),
    # ---- the same geometries on the large blocks ----
    _c("lg_c16_fsrcnn", "fwd", 1, (24, 16), 9, 4, 3, 1, (1, 17, 19), "k_conv_bfd<1,4,1,2,2,", env=BIG3, epi="bl", block=256,
       props="uneven_taps multi_tile"),
    _c("lg_c32_x6", "fwd", 1, (56, 32), 4, 2, 1, 0, (1, 19, 15), "k_conv_bfd<2,4,1,3,2,", algo="bf16x6", env=BIG, epi="b",
       block=256, props="multi_tile"),
    _c("lg_c48_f16", "fwd", 1, (80, 48), 3, 2, 1, 1, (1, 18, 17), "k_conv_bfd<3,4,1,2,1,", algo="f16x3", env=BIG, epi="bl",
       block=256, props="uneven_taps multi_tile"),
    _c("lg_c64", "fwd", 1, (64, 64), 5, 2, 2, 1, (1, 17, 16), "k_conv_bfd<4,4,1,2,1,", env=BIG3, epi="blr", block=256,
       props="uneven_taps multi_tile"),
    _c("lg_c64_x6_zero", "fwd", 1, (32, 64), 3, 4, 0, 0, (1, 12, 13), "k_conv_bfd<2,2,2,3,1,", algo="bf16x6", env=BIG,
       epi="blr", block=128, props="zero_tap multi_tile", exact="zero_tap"),
    _c("lg_c96_f16_zero", "fwd", 1, (32, 96), 2, 4, 0, 0, (1, 9, 16), "k_conv_bfd<2,2,2,2,1,", algo="f16x3", env=BIG,
       epi="blr", block=128, props="zero_tap multi_tile", exact="zero_tap"),
    _c("lg_c16_skipped", "fwd", 1, (8, 16), 3, 2, 1, 0, (2, 1, 40), "k_conv_bfd<1,4,1,2,2,", env=BIG3, epi="b", block=256,
       props="skipped uneven_taps"),
    # ---- k_conv_bf3: the kernels with the scalar-epilogue fallback (taken by bf3_cout10*: a 2-channel tail group, and by
    # bf3_prelu_c: per-channel slopes).  bf3_out_unaligned does NOT take it: epi_col_setup decides the 16-byte path from the
    # channel group alone, so that row checks k_conv_bf3's 16-byte phased stores (RS / CS with os = 4) to an address 4
    # bytes off a 16-byte boundary, next to the guards.  bf3_x_unaligned: scalar halo staging (vec_in = 0) ----
    _c("bf3_cout10", "fwd", 1, (24, 10), 4, 2, 1, 0, (2, 7, 6), "k_conv_bf3<1,1>", epi="bl", block=64),
    _c("bf3_prelu_c", "fwd", 1, (64, 64), 3, 2, 1, 1, (1, 9, 8), "k_conv_bf3<4,1>", epi="bPr", block=64,
       props="uneven_taps multi_tile"),
    _c("bf3_out_unaligned", "fwd", 1, (32, 32), 9, 4, 3, 1, (1, 5, 6), "k_conv_bf3<2,1>", epi="bl", off=(0, 4), block=64,
       props="uneven_taps"),
    _c("bf3_x_unaligned", "fwd", 1, (24, 16), 4, 2, 1, 0, (1, 6, 7), "k_conv_bf3<1,1>", env=(("SRK_BF3_DIRECT", "0"),),
       epi="b", off=(4, 0), block=64),
    _c("bf3_lds_filters_c64", "fwd", 1, (64, 64), 5, 2, 2, 1, (1, 17, 16), "k_conv_bf3<4,1>", env=BIG, epi="blr", block=64,
       props="uneven_taps multi_tile"),
    _c("bf3_cout10_zero", "fwd", 1, (24, 10), 2, 4, 0, 0, (1, 3, 4), "k_conv_bf3<1,1>", epi="blr", block=64,
       props="zero_tap", exact="zero_tap"),
    # ---- k_conv_tapn on strided TRANS gathers (Cin 32 / 64, Cout <= 3), bias + LeakyReLU + residual ----
    _c("tapn_k4s2", "fwd", 1, (64, 3), 4, 2, 1, 0, (2, 9, 7), "k_conv_tapn<2,3>", epi="blr", block=256, tol=TOL_TIGHT),
    _c("tapn_k4s2_x6", "fwd", 1, (64, 3), 4, 2, 1, 0, (2, 9, 7), "k_conv_tapn<2,3>", algo="bf16x6", epi="blr", block=256),
    _c("tapn_c32_1", "fwd", 1, (32, 1), 3, 2, 1, 1, (1, 11, 6), "k_conv_tapn<1,1>", epi="blr", block=256,
       props="uneven_taps", tol=TOL_TIGHT),
    _c("tapn_c32_1_x6", "fwd", 1, (32, 1), 3, 2, 1, 1, (1, 11, 6), "k_conv_tapn<1,1>", algo="bf16x6", epi="blr", block=256,
       props="uneven_taps"),
    _c("tapn_fsrcnn_d64", "fwd", 1, (64, 3), 9, 4, 3, 1, (1, 8, 5), "k_conv_tapn<2,3>", epi="blr", block=256,
       props="uneven_taps", tol=TOL_TIGHT),
    _c("tapn_fsrcnn_d64_x6", "fwd", 1, (64, 3), 9, 4, 3, 1, (1, 8, 5), "k_conv_tapn<2,3>", algo="bf16x6", epi="blr",
       block=256, props="uneven_taps"),
    _c("tapn_k9s2_groups", "fwd", 1, (64, 3), 9, 2, 4, 1, (1, 17, 18), "k_conv_tapn<2,3,multi,2>", epi="blr", block=256,
       props="uneven_taps multi_tile"),
    _c("tapn_k9s2_groups_x6", "fwd", 1, (64, 3), 9, 2, 4, 1, (1, 17, 18), "k_conv_tapn<2,3,multi,3>", algo="bf16x6",
       epi="blr", block=256, props="uneven_taps multi_tile"),
    _c("tapn_k2s4_zero", "fwd", 1, (64, 2), 2, 4, 0, 0, (2, 5, 6), "k_conv_tapn<2,2>", epi="blr", block=256,
       props="zero_tap", exact="zero_tap", tol=TOL_TIGHT),
    _c("tapn_k2s4_zero_x6", "fwd", 1, (64, 2), 2, 4, 0, 0, (2, 5, 6), "k_conv_tapn<2,2>", algo="bf16x6", epi="blr",
       block=256, props="zero_tap", exact="zero_tap"),
    # ---- k_conv_direct: the image deconvs of FSRCNN and LapSRN ----
    _c("direct_fsrcnn", "fwd", 1, (56, 3), 9, 4, 3, 1, (1, 23, 17), "k_conv_direct<3>", epi="b", block=256,
       props="uneven_taps multi_tile", tol=TOL_TIGHT),
    _c("direct_lapsrn_img", "fwd", 1, (3, 3), 4, 2, 1, 0, (1, 21, 14), "k_conv_direct<3>", epi="b", block=256,
       props="multi_tile", tol=TOL_TIGHT),
    # ---- the exact-fp32 MFMA kernels and the plain gather ----
    _c("mfma_tg_cin3", "fwd", 1, (3, 8), 4, 2, 1, 0, (2, 9, 7), "k_conv_mfma_tg<1>", epi="bl", block=128, tol=TOL_TIGHT),
    _c("cout6_plain_gather", "fwd", 1, (24, 6), 4, 2, 1, 0, (2, 7, 6), "k_gather_conv", epi="b", tol=TOL_TIGHT),
    _c("mfma_lapsrn_feat", "fwd", 1, (64, 64), 4, 2, 1, 0, (1, 13, 12), "k_conv_mfma<4>", algo="mfma_fp32", epi="bl",
       block=128, props="multi_tile"),
    _c("mfma_fsrcnn", "fwd", 1, (8, 8), 9, 4, 3, 1, (2, 11, 6), "k_conv_mfma<1>", algo="mfma_fp32", epi="b", block=128,
       props="uneven_taps"),
    _c("mfma_k3s4_zero", "fwd", 1, (80, 64), 3, 4, 0, 0, (1, 4, 5), "k_conv_mfma<4>", algo="mfma_fp32", epi="blr", block=128,
       props="zero_tap", exact="zero_tap"),
    _c("mfma_3x5", "fwd", 1, (56, 40), (3, 5), 2, 1, 0, (1, 7, 6), "k_conv_mfma<3>", algo="mfma_fp32", epi="b", block=128,
       props="uneven_taps"),
    _c("generic_k1_zero", "fwd", 1, (64, 64), 1, 2, 0, 1, (2, 6, 5), "k_gather_conv", algo="generic", epi="blr",
       props="zero_tap", exact="zero_tap"),
    _c("generic_k5_res", "fwd", 1, (64, 64), 5, 2, 2, 1, (1, 6, 7), "k_gather_conv", algo="generic", epi="r",
       props="uneven_taps"),
    _c("generic_1xW", "fwd", 1, (24, 8), 3, 2, 1, 0, (2, 1, 9), "k_gather_conv", algo="generic", epi="bl",
       props="skipped uneven_taps"),
    _c("generic_k5_s3", "fwd", 1, (24, 40), 5, 3, 2, 2, (1, 5, 7), "k_gather_conv", algo="generic", epi="lr",
       props="uneven_taps"),
    # ---- data gradient of strided convs: a TRANS gather over dy, with and without mask + add_to ----
    _c("dg_k3s2p1_even", "dgrad", 0, (64, 64), 3, 2, 1, 0, (2, 12, 10), _MP + "2>x4", block=64, props="uneven_taps"),
    _c("dg_k3s2p1_even_ma", "dgrad", 0, (64, 64), 3, 2, 1, 0, (2, 12, 10), _MP + "2>x4", epi="ma", block=64,
       props="uneven_taps"),
    _c("dg_k3s2p1_odd", "dgrad", 0, (24, 40), 3, 2, 1, 0, (1, 13, 9), "k_conv_bfd<1,1,2,2,2,", block=64, props="uneven_taps"),
    _c("dg_k3s2p1_odd_ma", "dgrad", 0, (24, 40), 3, 2, 1, 0, (1, 13, 9), "k_conv_bfd<1,1,2,2,2,", epi="ma", block=64,
       props="uneven_taps"),
    _c("dg_k4s2p1", "dgrad", 0, (64, 32), 4, 2, 1, 0, (1, 10, 14), _MP + "1>x4", block=64),
    _c("dg_k4s2p1_ma", "dgrad", 0, (64, 32), 4, 2, 1, 0, (1, 10, 14), _MP + "1>x4", epi="ma", block=64),
    _c("dg_k3s2p0_dead", "dgrad", 0, (40, 24), 3, 2, 0, 0, (2, 10, 13), "k_conv_bfd<1,1,3,2,2,", block=64,
       props="uneven_taps dead_rows", exact="dead"),
    _c("dg_k3s2p0_dead_ma", "dgrad", 0, (40, 24), 3, 2, 0, 0, (2, 10, 13), "k_conv_bfd<1,1,3,2,2,", epi="ma", block=64,
       props="uneven_taps dead_rows", exact="dead"),
    _c("dg_k3s2p0_dead_cols_a", "dgrad", 0, (40, 24), 3, 2, 0, 0, (1, 10, 14), "k_conv_bfd<1,1,3,2,2,", epi="a", block=64,
       props="uneven_taps dead_rows", exact="dead"),
    _c("dg_k1s2_zero", "dgrad", 0, (64, 64), 1, 2, 0, 0, (1, 9, 8), _MP + "2>x4", block=64, props="zero_tap", exact="dead"),
    _c("dg_k1s2_zero_ma", "dgrad", 0, (64, 64), 1, 2, 0, 0, (1, 9, 8), _MP + "2>x4", epi="ma", block=64, props="zero_tap",
       exact="dead"),
    _c("dg_k5s3p2", "dgrad", 0, (24, 56), 5, 3, 2, 0, (1, 11, 13), "k_conv_bfd<1,1,2,2,2,", block=64, props="uneven_taps"),
    _c("dg_k5s3p2_ma", "dgrad", 0, (24, 56), 5, 3, 2, 0, (1, 11, 13), "k_conv_bfd<1,1,2,2,2,", epi="ma", block=64,
       props="uneven_taps"),
    # Cin 3 <- Cout 64 (the first layer of a strided image conv): the masked taps-as-N kernel where its 32-column limit
    # allows (3x3: 27 columns), k_conv_direct otherwise (4x4: 48)
    _c("dg_img_k3_mask", "dgrad", 0, (3, 64), 3, 2, 1, 0, (2, 13, 10), "k_conv_tapn<2,3,mask>", epi="m", block=256,
       props="uneven_taps", tol=TOL_TIGHT),
    _c("dg_img_k4_mask", "dgrad", 0, (3, 64), 4, 2, 1, 0, (2, 12, 10), "k_conv_direct<3>", epi="m", block=256, tol=TOL_TIGHT),
    _c("dg_img_k4_a", "dgrad", 0, (3, 64), 4, 2, 1, 0, (2, 12, 10), "k_conv_tapn<2,3>", epi="a", block=256, tol=TOL_TIGHT),
    # ---- data gradient of transposed convs: a CONV gather with input stride s in the kernels ----
    _c("dgt_s2_small", "dgrad", 1, (24, 40), 4, 2, 1, 0, (2, 11, 7), "k_conv_bfd<1,1,2,2,2,", block=64, props="multi_tile"),
    _c("dgt_s4_small_a", "dgrad", 1, (64, 8), 9, 4, 3, 1, (1, 9, 10), "k_conv_bfd<1,1,4,2,2,", epi="a", block=64,
       props="multi_tile"),
    _c("dgt_s2_large", "dgrad", 1, (32, 24), 3, 2, 1, 1, (1, 19, 15), "k_conv_bfd<2,4,1,2,2,", env=BIG3, block=256,
       props="multi_tile"),
    _c("dgt_s4_large_ma", "dgrad", 1, (16, 56), 8, 4, 2, 0, (1, 17, 16), "k_conv_bfd<1,4,1,2,2,", env=BIG3, epi="ma",
       block=256, props="multi_tile"),
    _c("dgt_s2_x6", "dgrad", 1, (64, 64), 4, 2, 1, 0, (1, 9, 8), "k_conv_bfd<1,1,4,3,2,", algo="bf16x6", block=64,
       props="multi_tile"),
    # ---- weight gradient: k_wgrad_mfma<.,trans>, its strided non-transposed form, and the plain kernel ----
    # (exact fp32; beta 0 and beta 1 in every row.  wg_t_img: Cin <= 4 transposed has no MFMA plan, k_wgrad_generic sums its
    #  split partials with float atomics -- max-norm bar 1e-4, no bit-equality)
    _c("wg_t_k4s2_c64", "wgrad", 1, (64, 64), 4, 2, 1, 0, (2, 7, 6), "k_wgrad_mfma<4,trans>", tol=TOL_TIGHT),
    _c("wg_t_k9s4_fsrcnn", "wgrad", 1, (56, 8), 9, 4, 3, 1, (1, 6, 5), "k_wgrad_mfma<1,trans>", epi="n", tol=TOL_TIGHT),
    _c("wg_t_img", "wgrad", 1, (3, 3), 4, 2, 1, 0, (2, 10, 9), "k_wgrad_generic", tol=TOL_BF),
    _c("wg_k4s2", "wgrad", 0, (8, 16), 4, 2, 1, 0, (2, 14, 11), "k_wgrad_mfma<1,conv>", epi="n", tol=TOL_TIGHT),
    _c("wg_k4s2_img_smallcin", "wgrad", 0, (3, 16), 4, 2, 1, 0, (2, 14, 11), "k_wgrad_mfma_smallcin<5>", tol=TOL_TIGHT),
    _c("wg_k3s2p0_m", "wgrad", 0, (24, 40), 3, 2, 0, 0, (1, 10, 13), "k_wgrad_mfma<3,conv>", epi="m", tol=TOL_TIGHT),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
ATOMIC_ROWS = ("wg_t_img",)      # no bit-equality between two runs: float atomics


def dims(c):
    """(OH, OW) of the row's descriptor"""
    return out_dim(c.H, c.kh, c.s, c.p, c.tr, c.op), out_dim(c.W, c.kw, c.s, c.p, c.tr, c.op)


def gather(c):
    """the gather problem the kernels see: (trans, IH, IW, IC, OH, OW, OC); forward x -> y, data gradient dy -> dx"""
    OH, OW = dims(c)
    if c.kind == "dgrad":
        return int(not c.tr), OH, OW, c.cout, c.H, c.W, c.cin
    return c.tr, c.H, c.W, c.cin, OH, OW, c.cout


def case_phases(c):
    """the phases of a TRANS-gather row (None: a CONV gather or a weight gradient)"""
    if c.kind == "wgrad":
        return None
    trans, IH, IW, IC, OH, OW, OC = gather(c)
    return phases(c.kh, c.kw, c.s, c.p, OH, OW) if trans else None


def axis_reached(K, stride, pad, O, I):
    """per output index of one axis of a TRANS gather: does any tap of its phase read inside the input?  -> (reached [O],
    in a zero-tap phase [O])"""
    reached, zero = [False] * O, [False] * O
    for o0, P, Kv, i0, w0, wd in phases_1d(K, stride, pad, O):
        for r in range(P):
            o = o0 + r * stride
            zero[o] = Kv == 0
            reached[o] = any(0 <= r + i0 + u < I for u in range(Kv))
    return reached, zero


def properties(c):
    """the row's edges, recomputed from the library's phases"""
    props = set()
    if c.kind == "wgrad":
        return props
    trans, IH, IW, IC, OH, OW, OC = gather(c)
    if not trans:
        if c.block and OH * OW > c.block:
            props.add("multi_tile")
        return props
    ph = case_phases(c)
    if any(q.KHv * q.KWv == 0 for q in ph):
        props.add("zero_tap")
    if len(ph) < c.s * c.s:
        props.add("skipped")
    if len({q.KHv * q.KWv for q in ph if q.KHv * q.KWv}) > 1:
        props.add("uneven_taps")
    if c.block and any(q.PH * q.PW > c.block for q in ph):
        props.add("multi_tile")
    if c.kind == "dgrad":
        ry, zy = axis_reached(c.kh, c.s, c.p, OH, IH)
        rx, zx = axis_reached(c.kw, c.s, c.p, OW, IW)
        if any(not r and not z for r, z in zip(ry, zy)) or any(not r and not z for r, z in zip(rx, zx)):
            props.add("dead_rows")
    return props


def untouched(c):
    """[OH][OW] booleans of a TRANS-gather row: output pixels that no input reaches (zero-tap phases, dead rows / columns):
    the kernel's sum there is exactly zero"""
    trans, IH, IW, IC, OH, OW, OC = gather(c)
    assert trans
    ry, _ = axis_reached(c.kh, c.s, c.p, OH, IH)
    rx, _ = axis_reached(c.kw, c.s, c.p, OW, IW)
    return [[not (ry[y] and rx[x]) for x in range(OW)] for y in range(OH)]
