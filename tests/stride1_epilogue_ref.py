"""TEST INFRASTRUCTURE: the case table of the stride-1 convolution epilogue tests (tests/test_stride1_epilogue_cpu.py checks
the table's own conditions without a GPU, tests/test_stride1_epilogue_gpu.py runs it on the device through the C ABI).

A stride-1 Conv2d forward and its data gradient dispatch (csrc/api.hip run_gather) to one of about fifteen kernel families,
and every family ends in one of several store paths: the tile-affine 16-byte path (epi_store4_tile), the column-hoisted
16-byte path with its scalar fallback (epi_store4_col -> epi_store4 -> epi_store), the plain epi_store of the few-output-
channel kernels, and the private epilogues of the persistent kernels.  Which one a layer gets depends on the channel counts
and on facts a network never varies: Cout % 4, per-channel PReLU, the alignment of y / bias / residual, the run length of a
fused pixel shuffle.  CASES has one row per (family, block configuration, arithmetic, epilogue, alignment); a row STATES the
kernel it expects (`prefix`, compared with srk_last_kernel_name()) -- nothing here mirrors a dispatch predicate.

FAMILIES declares, as data, what each family's predicate accepts and what makes it decline (and to which family the layer
falls then); the CPU test asserts that every such pair has a row.

Shapes: two ragged tiles along each axis of the family's tile (8 x 8: (2, 13, 9); 16 x 16 / 256 pixels: (2, 19, 23);
8 x 16: (2, 13, 19)), N = 2 where the batch enters the addressing, one row per family narrower than a tile ((1, 3, 5));
the persistent kernels (k_conv_bfw, k_conv_bfr, k_conv_rowsw, k_conv_rowsr) at the smallest shapes tests/test_ops_gpu.py
forces them onto; k_conv_bf3's 2- and 4-wave blocks at the smallest problems the launcher gives them (65536 / 131072
pixels)."""
import collections

# kind: "fwd" srk_conv2d_forward_ex, "dgrad" srk_conv2d_backward_data (epi with X: srk_conv2d_backward_data_relu)
# algo: auto | generic | mfma_fp32 | direct | bf16x3 | bf16x6 | f16x3;  env: SRK_* switches set for the call
# epi, forward:  b bias;  R ReLU, l LeakyReLU(0.2), p PReLU (one slope), P PReLU (per channel), t tanh, s sigmoid;
#                n the PReLU slopes are negative;  r residual;  2 3 4 fused pixel shuffle ps_r (P behind it: Cout / r^2
#                slopes);  A y_amax given and the kernel keeps the maximum (wrote_amax == 1), Z y_amax given and it does not
#                (wrote_amax == 0, the slots untouched);  N x is NCHW (srk_conv_desc.x_nchw)
# epi, dgrad:    m LeakyReLU(0.2) mask on dy, z ReLU mask (slope 0);  a add_to;  2 4 dy_ps_r;  X the ReLU gradient of the
#                layer below on dx (srk_conv2d_backward_data_relu)
# off: bytes past a 16-byte boundary, "x4 y4 b4 r4": the gather's input (x / dy), its output (y / dx), bias, residual / add_to
# prefix: what srk_last_kernel_name() must start with; None: the call is refused (SRK_ERR_UNSUPPORTED, output untouched)
# decl: "family:option" -- the row is there because `option` makes `family` decline this layer
# tol: the bar, by the arithmetic that runs: 1e-4 bf16x3 class, 2e-5 (TOL_TIGHT) bf16x6 / f16x3 / exact fp32 / k_conv_tapn
#      with one tap group
Case = collections.namedtuple("Case", "id kind cin cout k p N H W algo env epi off prefix decl tol")

TOL_BF, TOL_TIGHT = 1e-4, 2e-5
S8, S16, S816, NARROW = (2, 13, 9), (2, 19, 23), (2, 13, 19), (1, 3, 5)

NOBFD = (("SRK_BF3_DIRECT", "0"),)                                 # bf16x3 small problems: k_conv_bf3 instead of k_conv_bfd
BIG = (("SRK_BFD_SMALL", "0"),)                                    # bf16x6 / f16x3: k_conv_bfd's large blocks
BIG3 = (("SRK_BFD_SMALL", "0"), ("SRK_BF3_DIRECT", "1"))           # bf16x3: the same
BFW = (("SRK_BFW", "1"), ("SRK_BF3_DIRECT", "0"), ("SRK_BFR", "0"))            # k_conv_bfw on small problems, no ring
RING = (("SRK_BFW", "1"), ("SRK_BF3_DIRECT", "0"), ("SRK_BFR", "1"), ("SRK_BFR_CV", "0"))
CANVAS = (("SRK_BFW", "1"), ("SRK_BF3_DIRECT", "0"), ("SRK_BFR", "1"), ("SRK_BFR_CV", "2"), ("SRK_C64", "0"))
ROWSW = (("SRK_ROWSW", "1"), ("SRK_ROWSR", "0"), ("SRK_ROWSB", "0"))
ROWSR = (("SRK_ROWSW", "1"), ("SRK_ROWSR", "1"), ("SRK_ROWSB", "0"))
ROWSB = (("SRK_ROWSW", "1"), ("SRK_ROWSR", "1"), ("SRK_ROWSB", "2"))
ROWN = (("SRK_ROWN", "2"),)

TIGHT_ALGOS = ("generic", "mfma_fp32", "direct", "bf16x6", "f16x3")


def _c(id, kind, ch, k, p, size, prefix, algo="auto", env=(), epi="", off="", decl=None, tol=None):
    if tol is None:
        tol = TOL_TIGHT if algo in TIGHT_ALGOS else TOL_BF
    offs = tuple(sorted((o[0], int(o[1:])) for o in off.split()))
    assert all(t in "xybr" and v in (0, 4, 8, 12) for t, v in offs)
    return Case(id, kind, ch[0], ch[1], k, p, size[0], size[1], size[2], algo, tuple(env), epi, offs, prefix, decl, tol)


def _sweep(stem, kind, ch, k, p, size, prefix, variants, amax="A", **kw):
    """one row per (tag, epi, off) of `variants` on one layer; amax="Z": the family never keeps the maximum"""
    return [_c("%s_%s" % (stem, tag), kind, ch, k, p, size, prefix, epi=epi.replace("A", amax), off=off, **kw)
            for tag, epi, off in variants]


# every epilogue a kernel with the scalar store path takes (each activation once, both PReLU forms with a negative slope
# once, bias / residual / y / x off a 16-byte boundary)
ALL_EPI = (("plain", "", ""), ("b_relu", "bRA", ""), ("lrelu_res", "lrA", ""), ("prelu1", "bp", ""), ("prelu1_neg", "pn", ""),
           ("preluC", "bP", ""), ("preluC_neg_res", "Pnr", ""), ("tanh", "bt", ""), ("sigmoid_res", "bsr", ""),
           ("b_off", "bl", "b4"), ("r_off", "br", "r4"), ("y_off", "bRZ", "y4"), ("x_off", "b", "x4"))
# ... and what a kernel compiled without it takes
VEC_EPI = (("plain", "", ""), ("b_relu", "bRA", ""), ("lrelu_res", "lrA", ""), ("prelu1", "bp", ""), ("prelu1_neg", "pn", ""),
           ("tanh", "bt", ""), ("sigmoid_res", "bsr", ""), ("x_off", "b", "x4"))
# what makes conv_epi_all_vector (csrc/conv_problem.h) say no
NONVEC = (("preluC", "bP", ""), ("b_off", "bl", "b4"), ("r_off", "br", "r4"), ("y_off", "bR", "y4"))

# data gradient: (no mask | LeakyReLU mask | ReLU mask) x (no add_to | aligned), and add_to 4 bytes off a 16-byte boundary
DG6 = (("plain", "", ""), ("m", "m", ""), ("z", "z", ""), ("a", "a", ""), ("ma", "ma", ""), ("za", "za", ""))
DG_OFF = (("a_off", "a", "r4"), ("ma_off", "ma", "r4"), ("za_off", "za", "r4"))

_BFD1, _BFD2, _BFD3, _BFD4 = ("k_conv_bfd<1,1,%d,2,2," % n for n in (1, 2, 3, 4))

CASES = (
    # ---- k_conv_bfd, small blocks (64 pixels x 1 .. 4 channel waves): the tile-affine 16-byte store ----
    _sweep("bfd_now2", "fwd", (24, 32), 3, 1, S8, _BFD2 + "1", VEC_EPI)
    + _sweep("bfd_now4_ksplit", "fwd", (64, 64), 3, 1, S8, _BFD4 + "2", VEC_EPI[1:])
    + [
        _c("bfd_now1", "fwd", (8, 16), 3, 1, S8, _BFD1 + "1", epi="blA"),
        _c("bfd_now3", "fwd", (40, 48), 3, 0, S8, _BFD3, epi="bprA"),
        _c("bfd_now1_narrow", "fwd", (16, 16), 3, 1, NARROW, _BFD1, epi="bRrA"),
        _c("bfd_k5", "fwd", (16, 32), 5, 2, S8, _BFD2, epi="blA"),
        _c("bfd_k1", "fwd", (32, 48), 1, 0, S8, _BFD3, epi="bR"),
        _c("bfd_ps2", "fwd", (24, 32), 3, 1, S8, _BFD2, epi="b2A"),
        _c("bfd_ps2_lrelu_res", "fwd", (64, 64), 3, 1, S8, _BFD4, epi="bl2rA"),
        _c("bfd_ps3_relu_res", "fwd", (24, 36), 3, 1, S8, _BFD3, epi="bR3r"),
        _c("bfd_ps4", "fwd", (32, 48), 3, 0, S8, _BFD3, epi="b4A"),
        _c("bfd_ps4_c1_prelu1", "fwd", (16, 16), 3, 1, S8, _BFD1, epi="bp4r"),
        _c("bfd_x6_now2", "fwd", (24, 32), 3, 1, S8, "k_conv_bfd<1,1,2,3,2,", algo="bf16x6", epi="bRrA"),
        _c("bfd_x6_now4_tanh", "fwd", (64, 64), 3, 1, S8, "k_conv_bfd<1,1,4,3,2,", algo="bf16x6", epi="bt"),
        _c("bfd_x6_ps2", "fwd", (16, 48), 3, 1, S8, "k_conv_bfd<1,1,3,3,2,", algo="bf16x6", epi="bp2rA"),
        _c("bfd_f16_now1", "fwd", (8, 16), 3, 1, S8, _BFD1, algo="f16x3", epi="blA"),
        _c("bfd_f16_now3_sigmoid", "fwd", (40, 48), 3, 1, S8, _BFD3, algo="f16x3", epi="bsr"),
        _c("bfd_f16_now4_ps2", "fwd", (64, 64), 3, 0, S8, _BFD4, algo="f16x3", epi="bR2rA"),
        # the large blocks (256 pixels; Cout 64 under bf16x6 / f16x3: 2 x 2 waves of 64 px x 32 ch)
        _c("bfd_lg_c16", "fwd", (24, 16), 3, 1, S16, "k_conv_bfd<1,4,1,2,2,", env=BIG3, epi="blA"),
        _c("bfd_lg_c32_x6", "fwd", (40, 32), 3, 1, S16, "k_conv_bfd<2,4,1,3,2,", algo="bf16x6", env=BIG, epi="bRr"),
        _c("bfd_lg_c48_f16", "fwd", (24, 48), 3, 1, S16, "k_conv_bfd<3,4,1,2,1,", algo="f16x3", env=BIG, epi="bprA"),
        _c("bfd_lg_c64", "fwd", (64, 64), 3, 1, S16, "k_conv_bfd<4,4,1,2,1,", env=BIG3, epi="btr"),
        _c("bfd_lg_c64_x6_ps2", "fwd", (32, 64), 3, 1, S16, "k_conv_bfd<2,2,2,3,1,", algo="bf16x6", env=BIG, epi="b2rA"),
        _c("bfd_lg_c64_f16", "fwd", (64, 64), 5, 2, S16, "k_conv_bfd<2,2,2,2,1,", algo="f16x3", env=BIG, epi="bsA"),
        _c("bfd_lg_c32_ps2_neg", "fwd", (24, 32), 3, 1, S16, "k_conv_bfd<2,4,1,2,2,", env=BIG3, epi="pn2A"),
        _c("bfd_lg_narrow", "fwd", (16, 32), 3, 1, NARROW, "k_conv_bfd<2,4,1,2,2,", env=BIG3, epi="bR"),
    ]
    # ---- what makes k_conv_bfd decline: k_conv_bf3 (bf16x3), k_conv_mfma (bf16x6), refused (f16x3) ----
    + [_c("bfd_decl_" + tag, "fwd", (24, 32), 3, 1, S8, "k_conv_bf3<2,1>", epi=epi, off=off, decl="bfd:" + opt)
       for (tag, epi, off), opt in zip(NONVEC, ("preluC", "bias_off", "res_off", "y_off"))]
    + [
        _c("bfd_decl_cout10", "fwd", (24, 10), 3, 1, S8, "k_conv_bf3<1,1>", epi="blZ", decl="bfd:cout_mod4"),
        _c("bfd_decl_ps2_ragged", "fwd", (24, 20), 3, 1, S8, "k_conv_bf3<2,1>", epi="b2r", decl="bfd:ps_ragged"),
        _c("bfd_decl_ps3_ragged", "fwd", (24, 18), 3, 1, S8, "k_conv_bf3<2,1>", epi="bR3r", decl="bfd:ps_ragged"),
        _c("bfd_decl_preluC_ps2", "fwd", (24, 32), 3, 1, S8, "k_conv_bf3<2,1>", epi="bP2", decl="bfd:preluC_ps"),
        _c("bfd_decl_x6_cout10", "fwd", (24, 10), 3, 1, S8, "k_conv_mfma<1>", algo="bf16x6", epi="bl", decl="bfd:cout_mod4"),
        _c("bfd_decl_x6_y_off", "fwd", (24, 32), 3, 1, S8, "k_conv_mfma<2>", algo="bf16x6", epi="bRZ", off="y4",
           decl="bfd:y_off"),
        _c("bfd_decl_f16_y_off", "fwd", (24, 32), 3, 1, S8, None, algo="f16x3", epi="bR", off="y4", decl="bfd:y_off"),
        _c("bfd_decl_f16_preluC", "fwd", (24, 32), 3, 1, S8, None, algo="f16x3", epi="bP", decl="bfd:preluC"),
    ]
    # ---- k_conv_bf3: the column-hoisted 16-byte store and its scalar fallback, 1-, 2- and 4-wave blocks ----
    + _sweep("bf3_nw1", "fwd", (24, 32), 3, 1, S8, "k_conv_bf3<2,1>", ALL_EPI, env=NOBFD, amax="Z")
    + [
        _c("bf3_nw1_c64_narrow", "fwd", (64, 64), 3, 1, NARROW, "k_conv_bf3<4,1>", env=NOBFD, epi="bRr"),
        _c("bf3_nw1_cout10_preluC", "fwd", (16, 10), 5, 2, S8, "k_conv_bf3<1,1>", epi="bPr"),
        _c("bf3_nw1_c48_ps4", "fwd", (32, 48), 3, 0, S8, "k_conv_bf3<3,1>", env=NOBFD, epi="bl4r"),
        _c("bf3_nw1_ps2_ragged_preluC", "fwd", (16, 20), 3, 1, S8, "k_conv_bf3<2,1>", epi="bPn2r"),
        _c("bf3_nw1_ps3_ragged_preluC", "fwd", (16, 18), 3, 1, S8, "k_conv_bf3<2,1>", epi="P3"),
        _c("bf3_nw1_ps3_tanh", "fwd", (16, 36), 3, 1, S8, "k_conv_bf3<3,1>", env=NOBFD, epi="bt3"),
        _c("bf3_nw2", "fwd", (8, 16), 3, 1, (1, 260, 255), "k_conv_bf3<1,2>", env=NOBFD, epi="bRrZ"),
        _c("bf3_nw4_vec", "fwd", (8, 32), 3, 1, (2, 258, 255), "k_conv_bf3<2,4,vec>", env=NOBFD + (("SRK_BFW", "0"),),
           epi="blrA"),
        _c("bf3_nw4_vec_ps2", "fwd", (8, 64), 3, 1, (2, 258, 255), "k_conv_bf3<4,4,vec>", env=NOBFD + (("SRK_BFW", "0"),),
           epi="bR2A"),
        _c("bf3_nw4_cout10", "fwd", (8, 10), 3, 1, (2, 258, 255), "k_conv_bf3<1,4>", epi="bPr"),
    ]
    # ---- k_conv_bf3_rows (Cin <= 4): 16-byte stores, ",scalar" where a group is not on them, ",f16" ----
    + _sweep("rows_c3", "fwd", (3, 32), 3, 1, S16, "k_conv_bf3_rows<2>", VEC_EPI)
    + _sweep("rows_c3_scalar", "fwd", (3, 32), 3, 1, S16, "k_conv_bf3_rows<2,scalar>", NONVEC)
    + [
        _c("rows_c1_cout24_scalar", "fwd", (1, 24), 5, 2, S16, "k_conv_bf3_rows<2,scalar>", epi="blrZ"),
        _c("rows_c3_cout10_scalar", "fwd", (3, 10), 3, 1, S16, "k_conv_bf3_rows<1,scalar>", epi="bPrZ", off="y4"),
        _c("rows_c4_c64_k5", "fwd", (4, 64), 5, 2, S16, "k_conv_bf3_rows<4>", epi="bRA"),
        _c("rows_c2_narrow", "fwd", (2, 16), 3, 1, NARROW, "k_conv_bf3_rows<1>", epi="brA"),
        _c("rows_c3_ps2", "fwd", (3, 32), 3, 1, S16, "k_conv_bf3_rows<2>", epi="bl2rA"),
        _c("rows_c3_ps2_ragged", "fwd", (3, 20), 3, 1, S16, "k_conv_bf3_rows<2,scalar>", epi="b2r"),
        _c("rows_c3_preluC_ps2", "fwd", (3, 32), 3, 1, S16, "k_conv_bf3_rows<2,scalar>", epi="bP2"),
        _c("rows_c3_nchw", "fwd", (3, 48), 3, 1, S16, "k_conv_bf3_rows<3>", epi="bRNA"),
        _c("rows_c3_f16", "fwd", (3, 32), 3, 1, S16, "k_conv_bf3_rows<2,f16>", algo="f16x3", epi="bprA"),
        _c("rows_c1_f16_nchw", "fwd", (1, 64), 5, 0, S16, "k_conv_bf3_rows<4,f16>", algo="f16x3", epi="btN"),
        _c("rows_f16_cout24", "fwd", (3, 24), 3, 1, S16, None, algo="f16x3", epi="bR", decl="bf3_rows_f16:cout_mod16"),
        _c("rows_f16_y_off", "fwd", (3, 32), 3, 1, S16, None, algo="f16x3", epi="bR", off="y4", decl="bf3_rows_f16:y_off"),
    ]
    # ---- k_conv_rowsw / k_conv_rowsr: the persistent first-layer kernels (private epilogues), forced onto small problems ----
    + [
        _c("rowsw_c4_c128", "fwd", (4, 128), 3, 1, (2, 17, 23), "k_conv_rowsw<", env=ROWSW, epi="bA"),
        _c("rowsw_c3_k5_relu", "fwd", (3, 64), 5, 2, (1, 19, 70), "k_conv_rowsw<", env=ROWSW, epi="bRA"),
        _c("rowsw_c1_lrelu", "fwd", (1, 64), 5, 2, (1, 19, 70), "k_conv_rowsw<", env=ROWSW, epi="bl"),
        _c("rowsw_c2_prelu1_neg", "fwd", (2, 64), 3, 0, (2, 17, 23), "k_conv_rowsw<", env=ROWSW, epi="bpn"),
        _c("rowsw_c3_f16_nchw", "fwd", (3, 64), 5, 0, (2, 21, 25), "k_conv_rowsw<", algo="f16x3", env=ROWSW, epi="bRNA"),
        _c("rowsr_c3_k3", "fwd", (3, 64), 3, 1, (2, 17, 23), "k_conv_rowsr<3>", env=ROWSR, epi="blA"),
        _c("rowsr_c3_k5_relu", "fwd", (3, 64), 5, 2, (2, 17, 23), "k_conv_rowsr<5,relu>", env=ROWSR, epi="bRA"),
        _c("rowsr_c4_c128_prelu1", "fwd", (4, 128), 3, 1, (2, 17, 23), "k_conv_rowsr<3>", env=ROWSR, epi="bp"),
        _c("rowsr_c1_f16_relu", "fwd", (1, 64), 5, 2, (2, 17, 23), "k_conv_rowsr<5,f16,relu>", algo="f16x3", env=ROWSR, epi="bRA"),
        _c("rowsr_c3_nchw", "fwd", (3, 64), 3, 1, (2, 17, 23), "k_conv_rowsr<3>", env=ROWSR, epi="bN"),
        _c("rowsw_ps2", "fwd", (3, 64), 3, 1, (2, 17, 23), "k_conv_rowsw<", env=ROWSW, epi="bl2A"),
        _c("rowsr_ps2_relu", "fwd", (3, 64), 3, 1, (2, 17, 23), "k_conv_rowsr<3,relu>", env=ROWSR, epi="bR2A"),
        _c("rowsr_band", "fwd", (3, 64), 3, 1, (2, 17, 23), "k_conv_rowsr<3,band>", env=ROWSB, epi="blA"),
        _c("rowsr_band_k5_relu", "fwd", (3, 64), 5, 2, (2, 17, 23), "k_conv_rowsr<5,relu,band>", env=ROWSB, epi="bRA"),
        _c("rowsw_decl_res", "fwd", (3, 64), 3, 1, (2, 17, 23), "k_conv_bf3_rows<4>", env=ROWSR, epi="br", decl="rowsw:res"),
        _c("rowsw_decl_tanh", "fwd", (3, 64), 3, 1, (2, 17, 23), "k_conv_bf3_rows<4>", env=ROWSR, epi="bt", decl="rowsw:tanh"),
        _c("rowsw_decl_sigmoid", "fwd", (3, 64), 3, 1, (2, 17, 23), "k_conv_bf3_rows<4>", env=ROWSW, epi="bs", decl="rowsw:sigmoid"),
        _c("rowsw_decl_preluC", "fwd", (3, 64), 3, 1, (2, 17, 23), "k_conv_bf3_rows<4,scalar>", env=ROWSR, epi="bP",
           decl="rowsw:preluC"),
        _c("rowsw_decl_y_off", "fwd", (3, 64), 3, 1, (2, 17, 23), "k_conv_bf3_rows<4,scalar>", env=ROWSW, epi="bR", off="y4",
           decl="rowsw:y_off"),
        _c("rowsw_decl_b_off", "fwd", (3, 64), 3, 1, (2, 17, 23), "k_conv_bf3_rows<4,scalar>", env=ROWSR, epi="bR", off="b4",
           decl="rowsw:bias_off"),
    ]
    # ---- k_conv_bfw (SRK_BFW=1): unrolled 3x3, dynamic taps, 64-pixel consumer waves, slices, pixel-shuffle store ----
    + [
        _c("bfw_3x3_c32", "fwd", (32, 32), 3, 1, (2, 19, 23), "k_conv_bfw<2,9,2>", env=BFW, epi="bRA"),
        _c("bfw_3x3_c16_lrelu", "fwd", (96, 16), 3, 1, (1, 19, 19), "k_conv_bfw<1,9,2>", env=BFW, epi="blA"),
        _c("bfw_5x5_prelu1", "fwd", (16, 32), 5, 2, (1, 20, 20), "k_conv_bfw<2,0,2>", env=BFW, epi="bp"),
        _c("bfw_5x5_prelu1_neg", "fwd", (16, 32), 5, 2, (1, 20, 20), "k_conv_bfw<2,0,2>", env=BFW, epi="pnA"),
        _c("bfw_1x1", "fwd", (32, 48), 1, 0, (3, 33, 9), "k_conv_bfw<3,0,2>", env=BFW, epi="b"),
        _c("bfw_c64_slices", "fwd", (40, 64), 3, 1, (2, 17, 23), "k_conv_bfw<2,9,2>", env=BFW, epi="bpA"),
        _c("bfw_c64_one_slice", "fwd", (32, 64), 3, 1, (2, 17, 23), "k_conv_bfw<4,0,4>", env=BFW, epi="bR"),
        _c("bfw_ps4", "fwd", (32, 48), 3, 0, (2, 21, 37), "k_conv_bfw<3,9,2>", env=BFW, epi="b4A"),
        _c("bfw_ps2_relu", "fwd", (32, 48), 3, 1, (1, 19, 23), "k_conv_bfw<3,9,2>", env=BFW, epi="bR2"),
        _c("bfw_f16", "fwd", (32, 32), 3, 1, (2, 19, 23), "k_conv_bfw<2,9,2,f16>", algo="f16x3", env=BFW, epi="bRA"),
        _c("bfw_decl_tanh", "fwd", (32, 32), 3, 1, (2, 19, 23), "k_conv_bf3<2,1>", env=BFW, epi="bt", decl="bfw:tanh"),
        _c("bfw_decl_sigmoid", "fwd", (32, 32), 3, 1, (2, 19, 23), "k_conv_bf3<2,1>", env=BFW, epi="bs", decl="bfw:sigmoid"),
        _c("bfw_decl_preluC", "fwd", (32, 32), 3, 1, (2, 19, 23), "k_conv_bf3<2,1>", env=BFW, epi="bP", decl="bfw:preluC"),
        _c("bfw_decl_y_off", "fwd", (32, 32), 3, 1, (2, 19, 23), "k_conv_bf3<2,1>", env=BFW, epi="bR", off="y4",
           decl="bfw:y_off"),
        _c("bfw_decl_b_off", "fwd", (32, 32), 3, 1, (2, 19, 23), "k_conv_bf3<2,1>", env=BFW, epi="bR", off="b4",
           decl="bfw:bias_off"),
        _c("bfw_decl_x_off", "fwd", (32, 32), 3, 1, (2, 19, 23), "k_conv_bf3<2,1>", env=BFW, epi="bR", off="x4",
           decl="bfw:x_off"),
        _c("bfw_decl_res", "fwd", (32, 32), 3, 1, (2, 19, 23), "k_conv_bf3<2,1>", env=BFW, epi="br", decl="bfw:res"),
        # the ring form, and its canvas variant: the only one of the family that adds a residual
        _c("bfr_ring_c32", "fwd", (32, 32), 3, 0, (1, 19, 19), "k_conv_bfr<2,1>", env=RING, epi="blA"),
        _c("bfr_ring_c32_2chunks", "fwd", (64, 32), 3, 0, (1, 11, 35), "k_conv_bfr<2,2>", env=RING, epi="bRA"),
        _c("bfr_ring_c48_ps4", "fwd", (32, 48), 3, 0, (2, 19, 19), "k_conv_bfr<3,1>", env=RING, epi="b4A"),
        _c("bfr_ring_f16_prelu1", "fwd", (40, 32), 3, 0, (2, 23, 17), "k_conv_bfr<2,2,f16>", algo="f16x3", env=RING, epi="bp"),
        _c("bfr_canvas_res", "fwd", (64, 64), 3, 1, (3, 13, 19), "k_conv_bfr<2,2,canvas,res>", env=CANVAS, epi="brA"),
        _c("bfr_canvas_relu", "fwd", (64, 64), 3, 1, (3, 13, 19), "k_conv_bfr<2,2,canvas>", env=CANVAS, epi="bRA"),
        _c("bfr_canvas_f16_res", "fwd", (64, 32), 3, 1, (3, 13, 19), "k_conv_bfr<2,2,f16,canvas,res>", algo="f16x3",
           env=CANVAS, epi="brA"),
        _c("bfr_canvas0_res", "fwd", (64, 64), 3, 1, (2, 16, 32), "k_conv_bfr<2,2,canvas0,res>", env=CANVAS, epi="br"),
        _c("bfr_canvas_decl_r_off", "fwd", (64, 64), 3, 1, (3, 13, 19), "k_conv_bf3<4,1>", env=CANVAS, epi="br", off="r4",
           decl="bfr:res_off"),
    ]
    # ---- k_c64 (64 -> 64, 3x3, pad 1, small problems): bias and / or residual only ----
    + [
        _c("c64_b", "fwd", (64, 64), 3, 1, S8, "k_c64<2,0>", epi="bA"),
        _c("c64_r", "fwd", (64, 64), 3, 1, S8, "k_c64<2,0>", epi="rA"),
        _c("c64_br_x6", "fwd", (64, 64), 3, 1, S8, "k_c64<3,0>", algo="bf16x6", epi="brA"),
        _c("c64_br_f16", "fwd", (64, 64), 3, 1, S8, "k_c64<2,0,f16>", algo="f16x3", epi="brA"),
        _c("c64_narrow", "fwd", (64, 64), 3, 1, NARROW, "k_c64<2,0>", epi="br"),
        _c("c64_decl_relu", "fwd", (64, 64), 3, 1, S8, _BFD4, epi="bRr", decl="c64:relu"),
        _c("c64_decl_x_off", "fwd", (64, 64), 3, 1, S8, _BFD4, epi="br", off="x4", decl="c64:x_off"),
        _c("c64_decl_ps2", "fwd", (64, 64), 3, 1, S8, _BFD4, epi="b2", decl="c64:ps_vec"),
        _c("c64_decl_y_off", "fwd", (64, 64), 3, 1, S8, "k_conv_bf3<4,1>", epi="br", off="y4", decl="c64:y_off"),
        _c("c64_decl_r_off", "fwd", (64, 64), 3, 1, S8, "k_conv_bf3<4,1>", epi="br", off="r4", decl="c64:res_off"),
        _c("c64_decl_b_off", "fwd", (64, 64), 3, 1, S8, "k_conv_bf3<4,1>", epi="b", off="b4", decl="c64:bias_off"),
        _c("c64_decl_x6_relu", "fwd", (64, 64), 3, 1, S8, "k_conv_bfd<1,1,4,3,2,", algo="bf16x6", epi="bR", decl="c64:relu"),
    ]
    # ---- k_conv_tapn (Cout <= 3, Cin 32 / 64): plain epi_store; one tap group (exact split: TOL_TIGHT) and several ----
    + _sweep("tapn_c64_3", "fwd", (64, 3), 3, 1, S16, "k_conv_tapn<2,3>", ALL_EPI[:-1], tol=TOL_TIGHT, amax="Z")
    + [
        _c("tapn_c32_1", "fwd", (32, 1), 3, 1, S16, "k_conv_tapn<1,1>", epi="btr", tol=TOL_TIGHT),
        _c("tapn_c32_2_x6", "fwd", (32, 2), 3, 0, S16, "k_conv_tapn<1,2>", algo="bf16x6", epi="bPn"),
        _c("tapn_narrow", "fwd", (64, 3), 3, 1, NARROW, "k_conv_tapn<2,3>", epi="bRr", tol=TOL_TIGHT),
        _c("tapn_multi", "fwd", (64, 3), 5, 2, S16, "k_conv_tapn<2,3,multi,2>", epi="bPrZ"),
        _c("tapn_multi_x6", "fwd", (64, 3), 5, 2, S16, "k_conv_tapn<2,3,multi,3>", algo="bf16x6", epi="bsr"),
        _c("tapn_multi_y_off", "fwd", (32, 3), 9, 4, S16, "k_conv_tapn<1,3,multi,2>", epi="bl", off="y4 b4"),
        _c("tapn_n2_res_y_off", "fwd", (64, 3), 3, 1, S16, "k_conv_tapn<2,3>", epi="blr", off="y4 r4", tol=TOL_TIGHT),
        _c("tapn_decl_x_off", "fwd", (64, 3), 3, 1, S16, "k_conv_direct<3>", epi="bR", off="x4", decl="tapn:x_off",
           tol=TOL_TIGHT),
    ]
    # ---- k_conv_rown (SRK_ROWN=2: Cout <= 3, more taps than one group, 5 / 7 / 9 columns) ----
    + _sweep("rown_k5", "fwd", (64, 3), 5, 2, S16, "k_conv_rown<2,3,5,2,", ALL_EPI[:-1], env=ROWN, amax="Z")
    + [
        _c("rown_k9_c32_x6", "fwd", (32, 3), 9, 4, S16, "k_conv_rown<1,3,9,3,", algo="bf16x6", env=ROWN, epi="bPr"),
        _c("rown_k7_c2", "fwd", (64, 2), 7, 3, (2, 13, 70), "k_conv_rown<2,2,7,2,", env=ROWN, epi="btr"),
        _c("rown_narrow", "fwd", (64, 3), 5, 2, NARROW, "k_conv_rown<2,3,5,2,", env=ROWN, epi="bR"),
        _c("rown_decl_x_off", "fwd", (64, 3), 5, 2, S16, "k_conv_direct<3>", env=ROWN, epi="bR", off="x4", decl="rown:x_off",
           tol=TOL_TIGHT),
    ]
    # ---- k_conv_direct (Cout <= 4, exact fp32) ----
    + _sweep("direct_c3", "fwd", (24, 3), 3, 1, S16, "k_conv_direct<3>", ALL_EPI, tol=TOL_TIGHT, amax="Z")
    + [
        _c("direct_c4_ps2", "fwd", (8, 4), 5, 2, S16, "k_conv_direct<4>", epi="bR2r", tol=TOL_TIGHT),
        _c("direct_c1_cin3", "fwd", (3, 1), 3, 1, S16, "k_conv_direct<1>", algo="direct", epi="bsr"),
        _c("direct_narrow", "fwd", (3, 3), 3, 1, NARROW, "k_conv_direct<3>", epi="bPr", tol=TOL_TIGHT),
        _c("direct_n2_res_y_off", "fwd", (8, 4), 3, 1, S16, "k_conv_direct<4>", epi="bpr", off="y4", tol=TOL_TIGHT),
        _c("direct_refused_cout8", "fwd", (24, 8), 3, 1, S8, None, algo="direct", epi="b", decl="direct:cout_gt4"),
    ]
    # ---- the exact-fp32 MFMA kernels: epi_store4_col with its scalar fallback ----
    + _sweep("mfma_c32", "fwd", (24, 32), 3, 1, S816, "k_conv_mfma<2>", ALL_EPI, algo="mfma_fp32")
    + [
        _c("mfma_cout10", "fwd", (16, 10), 3, 1, S816, "k_conv_mfma<1>", algo="mfma_fp32", epi="bPrZ"),
        _c("mfma_c64_ps2", "fwd", (64, 64), 3, 1, S816, "k_conv_mfma<4>", algo="mfma_fp32", epi="bl2rA"),
        _c("mfma_ps2_ragged", "fwd", (16, 20), 3, 1, S816, "k_conv_mfma<2>", algo="mfma_fp32", epi="bR2rZ"),
        _c("mfma_ps3_ragged_preluC", "fwd", (16, 18), 3, 1, S816, "k_conv_mfma<2>", algo="mfma_fp32", epi="bP3"),
        _c("mfma_ps4", "fwd", (16, 48), 3, 1, S816, "k_conv_mfma<3>", algo="mfma_fp32", epi="bt4r"),
        _c("mfma_narrow", "fwd", (16, 16), 3, 1, NARROW, "k_conv_mfma<1>", algo="mfma_fp32", epi="bRrA"),
    ]
    + _sweep("mfma_tg_cin3", "fwd", (3, 24), 3, 1, S816, "k_conv_mfma_tg<2>", ALL_EPI, algo="mfma_fp32")
    + [
        _c("mfma_cin5_auto", "fwd", (5, 16), 3, 1, S816, "k_conv_mfma<1>", epi="bRrA", tol=TOL_TIGHT),
        _c("mfma_cin6_cout10_auto", "fwd", (6, 10), 5, 2, S816, "k_conv_mfma<1>", epi="bPr", tol=TOL_TIGHT),
        _c("mfma_tg_cout10_narrow", "fwd", (4, 10), 5, 2, NARROW, "k_conv_mfma_tg<1>", algo="mfma_fp32", epi="bPr"),
        _c("mfma_tg_ps2_ragged", "fwd", (3, 20), 3, 1, S816, "k_conv_mfma_tg<2>", algo="mfma_fp32", epi="bR2rZ"),
        _c("mfma_tg_ps3_ragged_preluC", "fwd", (4, 18), 3, 1, S816, "k_conv_mfma_tg<2>", algo="mfma_fp32", epi="bPn3"),
        _c("mfma_tg_ps2", "fwd", (3, 32), 3, 1, S816, "k_conv_mfma_tg<2>", algo="mfma_fp32", epi="bl2rA"),
    ]
    # ---- k_gather_conv: algo generic, and Cout 5 .. 7 under auto ----
    + _sweep("generic_c32", "fwd", (24, 32), 3, 1, S8, "k_gather_conv", ALL_EPI, algo="generic", amax="Z")
    + [
        _c("generic_narrow", "fwd", (16, 16), 3, 1, NARROW, "k_gather_conv", algo="generic", epi="bPr", off="y4"),
        _c("generic_cout6_auto", "fwd", (24, 6), 3, 1, S8, "k_gather_conv", epi="bPrZ", tol=TOL_TIGHT),
        _c("generic_cout5_auto_y_off", "fwd", (16, 5), 5, 2, S8, "k_gather_conv", epi="btr", off="y4 r4", tol=TOL_TIGHT),
        _c("generic_cout7_auto", "fwd", (8, 7), 3, 1, S8, "k_gather_conv", epi="bl", tol=TOL_TIGHT),
        _c("generic_ps2_ragged", "fwd", (16, 20), 3, 1, S8, "k_gather_conv", algo="generic", epi="bP2r"),
        _c("generic_ps3", "fwd", (16, 18), 3, 1, S8, "k_gather_conv", algo="generic", epi="bs3"),
        _c("generic_ps4", "fwd", (16, 16), 3, 1, S8, "k_gather_conv", algo="generic", epi="bR4r"),
    ]
    # ---- data gradient of a stride-1 Conv2d (a TRANS gather over dy; (cin, cout) are the conv's): mask x add_to ----
    + _sweep("dg_bfd", "dgrad", (32, 24), 3, 1, S8, _BFD2, DG6 + (("dy_off", "m", "x4"),))
    + _sweep("dg_bfd_c64", "dgrad", (64, 64), 3, 1, S8, _BFD4 + "2", (("m", "m", ""), ("za", "za", "")))
    + _sweep("dg_bf3", "dgrad", (32, 24), 3, 1, S8, "k_conv_bf3<2,1>",
             DG_OFF + (("z_dx_off", "z", "y4"), ("ma_off_dx_off", "ma", "r4 y4")))
    + _sweep("dg_bf3_nobfd", "dgrad", (32, 24), 3, 1, S8, "k_conv_bf3<2,1>", DG6 + DG_OFF, env=NOBFD)
    + [
        _c("dg_bf3_cin10", "dgrad", (10, 24), 3, 1, S8, "k_conv_bf3<1,1>", epi="ma", decl="bfd:cout_mod4"),
        _c("dg_bfd_lg_c64", "dgrad", (64, 32), 3, 1, S16, "k_conv_bfd<4,4,1,2,1,", env=BIG3, epi="ma"),
        _c("dg_bfd_x6", "dgrad", (32, 24), 3, 1, S8, "k_conv_bfd<1,1,2,3,2,", algo="bf16x6", epi="za"),
        _c("dg_c64", "dgrad", (64, 64), 3, 1, S8, "k_c64<2,1>"),
        _c("dg_c64_a", "dgrad", (64, 64), 3, 1, S8, "k_c64<2,1>", epi="a"),
        _c("dg_c64_x6_a", "dgrad", (64, 64), 3, 1, S8, "k_c64<3,1>", algo="bf16x6", epi="a"),
        _c("dg_c64_decl_mask", "dgrad", (64, 64), 3, 1, S8, _BFD4, epi="z", decl="c64:mask"),
        _c("dg_c64_decl_a_off", "dgrad", (64, 64), 3, 1, S8, "k_conv_bf3<4,1>", epi="a", off="r4", decl="c64:res_off"),
    ]
    + _sweep("dg_bfw_mask", "dgrad", (64, 64), 3, 1, (2, 17, 23), "k_conv_bfw<2,9,2,mask>", (("m", "m", ""), ("z", "z", "")),
             env=BFW)
    + [
        _c("dg_bfw_mask_c32", "dgrad", (32, 64), 3, 1, (2, 17, 23), "k_conv_bfw<2,9,2,mask>", env=BFW, epi="m"),
        _c("dg_bfw_plain", "dgrad", (64, 64), 3, 1, (2, 17, 23), "k_conv_bfw<2,9,2>", env=BFW),
        _c("dg_bfw_decl_add", "dgrad", (64, 64), 3, 1, (2, 17, 23), "k_conv_bf3<4,1>", env=BFW, epi="ma", decl="bfw:res"),
        _c("dg_bfw_decl_a_off", "dgrad", (64, 64), 3, 1, (2, 17, 23), "k_conv_bf3<4,1>", env=BFW, epi="a", off="r4",
           decl="bfw:res_off"),
        _c("dg_bfr_canvas_add", "dgrad", (64, 64), 3, 1, (3, 13, 19), "k_conv_bfr<2,2,canvas,res>", env=CANVAS, epi="a"),
        # dx of a few-output-channel conv (Cin 16 .. 64 <- Cout <= 3): taps in K, one step (k_conv_tapk) or one per kernel row
        _c("dg_tapk", "dgrad", (64, 3), 3, 1, S16, "k_conv_tapk<4>"),
        _c("dg_tapk_a", "dgrad", (64, 3), 3, 1, (2, 13, 19), "k_conv_tapk<4>", epi="a"),
        _c("dg_tapk_c32_narrow", "dgrad", (32, 2), 3, 1, NARROW, "k_conv_tapk<2>", epi="a"),
        _c("dg_tapk_decl_mask", "dgrad", (64, 3), 3, 1, S16, "k_conv_mfma_tg<4>", epi="m", decl="tapk:mask", tol=TOL_TIGHT),
        _c("dg_tapk_decl_a_off", "dgrad", (64, 3), 3, 1, S16, "k_conv_mfma_tg<4>", epi="a", off="r4", decl="tapk:res_off",
           tol=TOL_TIGHT),
        _c("dg_tapk_decl_dx_off", "dgrad", (64, 3), 3, 1, S16, "k_conv_mfma_tg<4>", epi="a", off="y4", decl="tapk:y_off",
           tol=TOL_TIGHT),
        _c("dg_tapkm", "dgrad", (64, 3), 9, 4, S16, "k_conv_tapkm<4>"),
        _c("dg_tapkm_a", "dgrad", (64, 3), 9, 4, (2, 13, 19), "k_conv_tapkm<4>", epi="a"),
        _c("dg_tapkm_narrow", "dgrad", (64, 3), 9, 4, NARROW, "k_conv_tapkm<4>", epi="a"),
        _c("dg_tapkm_k5_c32", "dgrad", (32, 3), 5, 2, S16, "k_conv_tapkm<2>", epi="a"),
        _c("dg_tapkm_decl_mask", "dgrad", (64, 3), 9, 4, S16, "k_conv_mfma_tg<4>", epi="za", decl="tapkm:mask", tol=TOL_TIGHT),
        _c("dg_tapkm_decl_a_off", "dgrad", (64, 3), 9, 4, S16, "k_conv_mfma_tg<4>", epi="a", off="r4", decl="tapkm:res_off",
           tol=TOL_TIGHT),
        # dx of a first layer (Cin <= 3 <- Cout 32 / 64): k_conv_tapn, with the mask prologue while the taps fit one group
        _c("dg_tapn_img", "dgrad", (3, 64), 3, 1, S16, "k_conv_tapn<2,3>", epi="a", tol=TOL_TIGHT),
        _c("dg_tapn_img_mask", "dgrad", (3, 64), 3, 1, S16, "k_conv_tapn<2,3,mask>", epi="ma", tol=TOL_TIGHT),
        _c("dg_tapn_img_relu_mask", "dgrad", (3, 32), 3, 1, S16, "k_conv_tapn<1,3,mask>", epi="z", off="y4", tol=TOL_TIGHT),
    ]
    + _sweep("dg_mfma", "dgrad", (32, 24), 3, 1, S816, "k_conv_mfma<2>", DG6 + DG_OFF + (("m_dx_off", "m", "y4"),),
             algo="mfma_fp32")
    + _sweep("dg_generic", "dgrad", (32, 24), 3, 1, S8, "k_gather_conv", DG6 + DG_OFF + (("m_dx_off", "m", "y4"),),
             algo="generic")
    # dy in the pixel-shuffled layout (dy_ps_r): both kernels run_gather picks
    + _sweep("dg_ps2_bfd", "dgrad", (16, 32), 3, 1, S8, _BFD1, (("plain", "2", ""), ("ma", "ma2", ""), ("z", "z2", "")))
    + _sweep("dg_ps4_bfd", "dgrad", (24, 128), 3, 1, S8, _BFD2, (("plain", "4", ""), ("za", "za4", "")))
    + _sweep("dg_ps2_bf3", "dgrad", (16, 32), 3, 1, S8, "k_conv_bf3<1,1>", (("plain", "2", ""), ("ma", "ma2", "")), env=BIG)
    + [
        _c("dg_ps4_bf3_a_off", "dgrad", (24, 128), 3, 1, S8, "k_conv_bf3<2,1>", epi="ma4", off="r4"),
        _c("dg_ps2_refused_x6", "dgrad", (16, 32), 3, 1, S8, None, algo="bf16x6", epi="2", decl="dy_ps:algo"),
        # srk_conv2d_backward_data_relu: ReLU gradient of the layer below on dx; with the mask on dy; refused
        _c("dg_relu", "dgrad", (64, 64), 3, 1, (2, 17, 23), "k_conv_bfw<2,9,2,relu>", env=BFW, epi="X"),
        _c("dg_mask_relu", "dgrad", (64, 64), 3, 1, (2, 17, 23), "k_conv_bfw<2,9,2,mask,relu>", env=BFW, epi="zX"),
        _c("dg_lmask_relu_c32", "dgrad", (32, 64), 3, 1, (2, 17, 23), "k_conv_bfw<2,9,2,mask,relu>", env=BFW, epi="mX"),
        _c("dg_relu_refused_5x5", "dgrad", (64, 32), 5, 2, (2, 17, 23), None, env=BFW, epi="X", decl="relu_out:taps"),
        _c("dg_relu_refused_small", "dgrad", (64, 64), 3, 1, (2, 17, 23), None, epi="X", decl="relu_out:size"),
    ]
)
BY_ID = {c.id: c for c in CASES}

# ---- what each family's predicate accepts, and what makes it decline (option -> the family the layer falls to) ----
# Read once from: run_gather csrc/api.hip:182-276;  conv_epi_all_vector csrc/conv_problem.h:103-115 (cout_mod4, preluC,
# y_off / bias_off / res_off, ps_ragged);  conv_bfd_gather_supported csrc/conv_bfd.hip:741-748;  conv_bf3_gather_supported
# csrc/conv_mfma_bf16.hip:900-908, bf3_launch_rows :917-924, conv_bf3_rows_f16_supported :1033-1036;  conv_rowsw_applicable
# csrc/conv_rowsw.hip:728-743;  conv_bfw_applicable csrc/conv_bfw.hip:486-515, conv_bfr_canvas / conv_bfr_launch
# csrc/conv_bfr.hip:639-752;  conv_c64_applicable csrc/conv_c64.hip:263-271;  conv_tapn_gather_supported
# csrc/conv_tapn.hip:206-214, conv_tapk_ / conv_tapkm_gather_supported :692-701 / :904-914;  conv_rown_gather_supported
# csrc/conv_rown.hip:262-275;  conv_mfma_ / conv_direct_gather_supported csrc/conv_mfma.hip:427-433 / :549-552
# (line numbers as of the commit that added this table).
# A fused pixel shuffle with r = 4 has runs of 4 * Cout/16 floats, always a multiple of 4: only r = 2 and r = 3 have a
# ragged form.  Families whose Cout is a multiple of 16 (bfw, rowsw) cannot see cout_mod4 or ps_ragged.
_ACTS = ("relu", "lrelu", "prelu1", "tanh", "sigmoid", "neg_slope")
_ANY = _ACTS + ("bias", "res", "preluC", "bias_off", "res_off", "y_off", "amax")
_MASKS = ("mask", "mask0", "add")
FAMILIES = {
    "bfd": dict(accepts=_ACTS + ("bias", "res", "x_off", "ps_vec", "amax") + _MASKS + ("dy_ps",),
                declines={"cout_mod4": ("bf3", "mfma"), "preluC": ("bf3", "refused"), "bias_off": ("bf3",),
                          "res_off": ("bf3",), "y_off": ("bf3", "mfma", "refused"), "ps_ragged": ("bf3",),
                          "preluC_ps": ("bf3",)}),
    "bf3": dict(accepts=_ANY + ("x_off", "cout_mod4", "ps_vec", "ps_ragged", "preluC_ps") + _MASKS + ("add_off", "dy_ps"),
                declines={}),
    "bf3_rows": dict(accepts=_ANY + ("x_off", "ps_vec", "ps_ragged", "preluC_ps", "x_nchw", "cout_mod16", "cout_mod4"),
                     declines={}),
    "bf3_rows_f16": dict(accepts=(), declines={"cout_mod16": ("refused",), "y_off": ("refused",)}),
    "rowsw": dict(accepts=("bias", "relu", "lrelu", "prelu1", "neg_slope", "ps_vec", "amax", "x_nchw"),
                  declines={"res": ("bf3_rows",), "tanh": ("bf3_rows",), "sigmoid": ("bf3_rows",), "preluC": ("bf3_rows",),
                            "y_off": ("bf3_rows",), "bias_off": ("bf3_rows",)}),
    "rowsr": dict(accepts=("bias", "relu", "lrelu", "prelu1", "ps_vec", "amax", "x_nchw"), declines={}),
    "bfw": dict(accepts=("bias", "relu", "lrelu", "prelu1", "neg_slope", "ps_vec", "amax", "mask", "mask0", "relu_out"),
                declines={"tanh": ("bf3",), "sigmoid": ("bf3",), "preluC": ("bf3",), "y_off": ("bf3",), "bias_off": ("bf3",),
                          "x_off": ("bf3",), "res": ("bf3",), "res_off": ("bf3",)}),
    "bfr": dict(accepts=("bias", "relu", "lrelu", "prelu1", "ps_vec", "amax", "res", "add"), declines={"res_off": ("bf3",)}),
    "c64": dict(accepts=("bias", "res", "amax", "add"),
                declines={"relu": ("bfd",), "x_off": ("bfd",), "ps_vec": ("bfd",), "y_off": ("bf3",), "res_off": ("bf3",),
                          "bias_off": ("bf3",), "mask": ("bfd",)}),
    "tapn": dict(accepts=_ANY + ("mask", "mask0", "add"), declines={"x_off": ("direct",)}),
    "rown": dict(accepts=_ANY, declines={"x_off": ("direct",)}),
    "direct": dict(accepts=_ANY + ("x_off", "ps_ragged"), declines={"cout_gt4": ("refused",)}),
    "mfma": dict(accepts=_ANY + ("x_off", "cout_mod4", "ps_vec", "ps_ragged", "preluC_ps") + _MASKS + ("add_off",), declines={}),
    "mfma_tg": dict(accepts=_ANY + ("x_off", "cout_mod4", "ps_vec", "ps_ragged", "preluC_ps"), declines={}),
    "generic": dict(accepts=_ANY + ("x_off", "ps_vec", "ps_ragged", "preluC_ps") + _MASKS + ("add_off",), declines={}),
    "tapk": dict(accepts=("add",), declines={"mask": ("mfma_tg",), "res_off": ("mfma_tg",), "y_off": ("mfma_tg",)}),
    "tapkm": dict(accepts=("add",), declines={"mask": ("mfma_tg",), "res_off": ("mfma_tg",)}),
    "dy_ps": dict(accepts=(), declines={"algo": ("refused",)}),
    "relu_out": dict(accepts=(), declines={"taps": ("refused",), "size": ("refused",)}),
}

_PREFIX_FAMILY = (("k_conv_bfd<", "bfd"), ("k_conv_bf3_rows<", "bf3_rows"), ("k_conv_bf3<", "bf3"), ("k_conv_rowsw<", "rowsw"),
                  ("k_conv_rowsr<", "rowsr"), ("k_conv_bfw<", "bfw"), ("k_conv_bfr<", "bfr"), ("k_c64<", "c64"),
                  ("k_conv_tapn<", "tapn"), ("k_conv_rown<", "rown"), ("k_conv_direct<", "direct"),
                  ("k_conv_mfma_tg<", "mfma_tg"), ("k_conv_mfma<", "mfma"), ("k_gather_conv", "generic"),
                  ("k_conv_tapkm<", "tapkm"), ("k_conv_tapk<", "tapk"))


def family(c):
    """the family the row expects to run ("refused": none)"""
    if c.prefix is None:
        return "refused"
    for p, f in _PREFIX_FAMILY:
        if c.prefix.startswith(p):
            return f
    raise KeyError(c.prefix)


def ps_r(c):
    """the fused pixel shuffle of a forward row / dy_ps_r of a data-gradient row (0: none)"""
    d = [int(ch) for ch in c.epi if ch in "234"]
    assert len(d) <= 1
    return d[0] if d else 0


def off(c, which):
    return dict(c.off).get(which, 0)


def act(c):
    """none | relu | lrelu | prelu1 | preluC | tanh | sigmoid"""
    names = {"R": "relu", "l": "lrelu", "p": "prelu1", "P": "preluC", "t": "tanh", "s": "sigmoid"}
    a = [names[ch] for ch in c.epi if ch in names] if c.kind == "fwd" else []
    assert len(a) <= 1
    return a[0] if a else "none"


def out_hw(c):
    """(OH, OW) of the stride-1 Conv2d"""
    return c.H + 2 * c.p - c.k + 1, c.W + 2 * c.p - c.k + 1


def options(c):
    """the option names (FAMILIES' vocabulary) the row exercises"""
    o, r = set(), ps_r(c)
    if off(c, "x"):
        o.add("x_off")
    if off(c, "y"):
        o.add("y_off")
    if c.kind == "fwd":
        a = act(c)
        if a != "none":
            o.add(a)
        if "n" in c.epi:
            o.add("neg_slope")
        if "b" in c.epi:
            o.add("bias_off" if off(c, "b") else "bias")
        if "r" in c.epi:
            o.add("res_off" if off(c, "r") else "res")
        if r:
            o.add("ps_vec" if (r * (c.cout // (r * r))) % 4 == 0 else "ps_ragged")
            if a == "preluC":
                o.add("preluC_ps")
        if c.cout % 4:
            o.add("cout_mod4")
        if c.cout % 16:
            o.add("cout_mod16")
        if "A" in c.epi or "Z" in c.epi:
            o.add("amax")
        if "N" in c.epi:
            o.add("x_nchw")
    else:
        if "m" in c.epi:
            o.add("mask")
        if "z" in c.epi:
            o.add("mask0")
        if "a" in c.epi:
            o.add("add_off" if off(c, "r") else "add")
        if r:
            o.add("dy_ps")
        if "X" in c.epi:
            o.add("relu_out")
        if c.cin % 4:
            o.add("cout_mod4")      # (the gather's output channels are the conv's input channels)
    return o


# option names under which a declining row may carry its `decl` option (data-gradient rows name the fan-in add_to)
DECL_ALIAS = {"add": "res", "add_off": "res_off", "mask0": "mask"}
SLOPE = 0.2


# ---- inputs and the float64 reference (torch on the CPU; imported on first use) ------------------------------------------
def shuffle_bias(b, r):
    """srk_pack_bias_ps: torch's channel c*r^2 + i*r + j at packed position (i*r + j)*C + c"""
    return b.view(-1, r * r).t().reshape(-1).contiguous() if r > 1 else b


_cache = {}


def tensors(cid):
    """float32, NCHW index order, as a dict: x, w (torch layout), b, pw (PReLU slopes: 1 or Cout / r^2), res (residual /
    add_to, of the call's output shape), dy, ym (the mask source, dy's shape), xr (x_relu, dx's shape)"""
    import torch
    from oracle import fill
    from conv_abi import _edges_x4
    if cid in _cache:
        return _cache[cid]
    c = BY_ID[cid]
    r = ps_r(c)
    OH, OW = out_hw(c)
    seed = 31000 + 20 * [k.id for k in CASES].index(cid)
    squash = act(c) in ("tanh", "sigmoid")
    fan = (c.cin if c.kind == "fwd" else c.cout) * c.k * c.k
    gain = 0.15 if squash else 2.0          # (tanh / sigmoid rows: pre-activations inside the part of the curve that bends)
    t = dict(x=_edges_x4(fill.randn((c.N, c.cin, c.H, c.W), seed)),
             w=fill.randn((c.cout, c.cin, c.k, c.k), seed + 1, (gain / fan) ** 0.5),
             b=fill.randn((c.cout,), seed + 2, 0.1))
    n_slopes = 1 if "p" in c.epi else (c.cout // (r * r) if r else c.cout)
    pw = 0.25 + 0.05 * fill.randn((n_slopes,), seed + 3)
    t["pw"] = -pw if "n" in c.epi else pw
    if c.kind == "fwd":
        out_shape = (c.N, c.cout // (r * r), OH * r, OW * r) if r else (c.N, c.cout, OH, OW)
        t["res"] = fill.randn(out_shape, seed + 4, 0.25 if squash else 0.5)
    else:
        t["res"] = fill.randn((c.N, c.cin, c.H, c.W), seed + 4, 0.5)
        t["dy"] = _edges_x4(fill.randn((c.N, c.cout, OH, OW), seed + 5))
        t["ym"] = _edges_x4(fill.randn((c.N, c.cout, OH, OW), seed + 6))
        t["xr"] = fill.randn((c.N, c.cin, c.H, c.W), seed + 7)
    if len(_cache) >= 4:
        _cache.clear()
    _cache[cid] = t
    return t


def compute(cid, dtype):
    """the row's operation with torch on the CPU in `dtype` -> dict of NCHW tensors: out (what the call must store; forward
    pixel-shuffle rows in the shuffled layout), term (out without the residual / add_to), pre (what the activation or the
    mask decides on; None: none)"""
    import torch
    import torch.nn.functional as F
    c = BY_ID[cid]
    t = {k: v.to(dtype) for k, v in tensors(cid).items()}
    r = ps_r(c)
    if c.kind == "fwd":
        z = F.conv2d(t["x"], t["w"], t["b"] if "b" in c.epi else None, 1, c.p)
        if r:
            z = F.pixel_shuffle(z, r)      # (the activations are element-wise: act, then shuffle == shuffle, then act)
        a = act(c)
        if a == "relu":
            y = torch.relu(z)
        elif a == "lrelu":
            y = F.leaky_relu(z, SLOPE)
        elif a in ("prelu1", "preluC"):
            y = F.prelu(z, t["pw"])
        elif a == "tanh":
            y = torch.tanh(z)
        elif a == "sigmoid":
            y = torch.sigmoid(z)
        else:
            y = z
        return dict(out=y + t["res"] if "r" in c.epi else y, term=y, pre=z if a != "none" else None)
    dy, pre = t["dy"], None
    if "m" in c.epi or "z" in c.epi:
        pre = t["ym"]
        dy = torch.where(pre > 0, dy, dy * (SLOPE if "m" in c.epi else 0.0))
    x = t["x"].clone().requires_grad_(True)
    F.conv2d(x, t["w"], None, 1, c.p).backward(dy)
    dx = x.grad
    if "X" in c.epi:
        pre = t["xr"] if pre is None else pre
        dx = dx * (t["xr"] > 0).to(dtype)
    return dict(out=dx + t["res"] if "a" in c.epi else dx, term=dx, pre=pre)


def reference(cid):
    """compute(cid, float64): one test per row asks for it, so nothing is kept"""
    import torch
    return compute(cid, torch.float64)
