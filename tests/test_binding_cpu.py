"""The ctypes binding is derived from include/srk.h (_header.py); these tests hold the derivation against the host C
compiler and the public surface against literals.  No GPU.

One generated translation unit includes the header.  Run, it prints sizeof of every struct, offsetof and size of every
field and the value of every constant, which are compared with the ctypes classes and the parsed table; compiled with
CHECK_SIGNATURES, it assigns every function to a pointer of the type the reader tokenised, and a mismatch is an error.
The reader's refusals are fed synthetic headers.  The expected constants below are literals on purpose: they are the
check of the derived values, not their source."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CC = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
needs_cc = pytest.mark.skipif(CC is None, reason="no host C compiler (cc, gcc, clang)")


@pytest.fixture(scope="module")
def pkg():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    return p


@pytest.fixture(scope="module")
def header(pkg):
    return pkg._header.read_file(pkg._lib.HEADER_PATH)


def unit_text(header, spellings=None):
    """The translation unit: layout and constant prints in main(), the signature pointers under CHECK_SIGNATURES."""
    out = ["#include <stddef.h>", "#include <stdio.h>", '#include "srk.h"', "#ifdef CHECK_SIGNATURES"]
    for name, (ret, params) in (spellings or header.spellings).items():
        out.append("%s (*const check_%s)(%s) = %s;" % (ret, name, ", ".join(params) or "void", name))
    out += ["#else", "int main(void) {"]
    for struct, fields in header.structs.items():
        out.append('  printf("sizeof %s - %%zu 0\\n", sizeof(%s));' % (struct, struct))
        for field, _ in fields:
            out.append('  printf("field %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));'
                       % (struct, field, struct, field, struct, field))
    for name in header.constants:
        out.append('  printf("const %s - %%lld 0\\n", (long long)%s);' % (name, name))
    out += ["  return 0;", "}", "#endif", ""]
    return "\n".join(out)


def check_signatures(path):
    return subprocess.run([CC, "-std=c99", "-fsyntax-only", "-DCHECK_SIGNATURES", "-Werror=incompatible-pointer-types",
                           "-I", INCLUDE, str(path)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def unit(header, tmp_path_factory):
    path = tmp_path_factory.mktemp("binding") / "probe.c"
    path.write_text(unit_text(header))
    return path


@pytest.fixture(scope="module")
def probe(unit):
    """{(kind, struct or constant, field or "-"): (offset or value, size)} as the compiled unit prints it."""
    exe = unit.with_suffix("")
    subprocess.run([CC, "-std=c99", "-I", INCLUDE, str(unit), "-o", str(exe)], check=True, capture_output=True, text=True)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    return {tuple(r.split()[:3]): tuple(int(v) for v in r.split()[3:]) for r in rows if r}


@needs_cc
def test_struct_layouts_match_the_compiler(pkg, header, probe):
    L = pkg._lib
    named = {"srk_conv_desc": L.ConvDesc, "srk_epilogue": L.Epilogue, "srk_conv_result": L.ConvResult,
             "srk_bwd_mask": L.BwdMask, "srk_wgrad_plan": L.WgradPlan, "srk_dense_desc": L.DenseDesc,
             "srk_dense_epilogue": L.DenseEpilogue, "srk_dense_plan": L.DensePlan, "srk_spectral_layer": L.SpectralLayer,
             "srk_phase_axis": L.PhaseAxis, "srk_phase": L.Phase}
    assert set(named) == set(header.structs)
    n_fields = 0
    for struct, fields in header.structs.items():
        for cls in (header.classes[struct], named[struct]):
            assert issubclass(cls, ctypes.Structure)
            assert probe[("sizeof", struct, "-")][0] == ctypes.sizeof(cls), struct      # a dropped field shows here
            assert list(cls._fields_) == fields
            for field, _ in fields:
                d = getattr(cls, field)
                assert probe[("field", struct, field)] == (d.offset, d.size), (struct, field)
        n_fields += len(fields)
    assert n_fields == 130 and len([k for k in probe if k[0] == "field"]) == n_fields
    assert {s: ctypes.sizeof(c) for s, c in named.items()} == {
        "srk_conv_desc": 64, "srk_epilogue": 64, "srk_conv_result": 12, "srk_bwd_mask": 16, "srk_wgrad_plan": 240,
        "srk_dense_desc": 72, "srk_dense_epilogue": 24, "srk_dense_plan": 40, "srk_spectral_layer": 48,
        "srk_phase_axis": 28, "srk_phase": 52}
    assert L.WgradPlan.name.size == 64 and L.WgradPlan.name.offset == 176
    assert dict(L.Epilogue._fields_)["bias"] is ctypes.c_void_p and dict(L.Epilogue._fields_)["bn_partial"] is ctypes.c_void_p


@needs_cc
def test_constants_match_the_compiler(header, probe):
    assert len(header.constants) == 60
    for name, value in header.constants.items():
        assert probe[("const", name, "-")][0] == value, name


@needs_cc
def test_signatures_match_the_compiler(header, unit, tmp_path):
    assert len(header.spellings) == len(header.functions) == 195
    for name, (_, params) in header.spellings.items():
        assert len(params) == len(header.functions[name][1]), name
    r = check_signatures(unit)
    assert r.returncode == 0, r.stderr
    # the check has teeth: a lost parameter and a narrowed one are both refused by the compiler
    ret, params = header.spellings["srk_img_resize_u8"]
    assert params[1] == "int64_t"
    for broken in (params[:-1], [params[0], "int"] + params[2:]):
        bad = tmp_path / "bad.c"
        bad.write_text(unit_text(header, dict(header.spellings, srk_img_resize_u8=(ret, broken))))
        r = check_signatures(bad)
        assert r.returncode != 0 and "check_srk_img_resize_u8" in r.stderr, r.stderr


def test_argtypes_follow_the_pointer_rule(pkg, header):
    L = pkg._lib
    assert L._PROTOTYPES is not None and set(L._PROTOTYPES) == set(header.functions) == set(L.header_symbols())
    scalars = set(pkg._header.SCALARS.values())
    struct_pointers = {ctypes.POINTER(c) for c in L._H.classes.values()}
    for name, (restype, argtypes) in L._PROTOTYPES.items():
        assert restype in scalars or restype is ctypes.c_char_p, name
        for t in argtypes:
            assert t in scalars or t is ctypes.c_void_p or t in struct_pointers, (name, t)
    P = L._PROTOTYPES
    vp, i, i64, f, d, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
    assert P["srk_version"] == (i, []) and P["srk_status_string"] == (ctypes.c_char_p, [i])
    assert P["srk_window_attention_token_pixel"] == (i64, [i] * 7)
    assert P["srk_packed_weight_bytes"] == (sz, [i] * 5)
    assert P["srk_pack_weights_batched"] == (i, [vp, vp, vp, i, i, vp, i, vp])          # const int64_t* table: a DEVICE pointer
    assert P["srk_bn_finalize"] == (i, [vp, d, vp, vp, vp, vp, f, f, i, vp, vp])
    assert P["srk_noise_u8"] == (i, [vp, vp, vp, ctypes.c_uint64, i, i64, vp])
    assert P["srk_vgg_tap_plan"] == (i, [i] * 6 + [vp])                                  # long long*
    assert P["srk_conv2d_backward_weight_grouped"][1][2:4] == [vp, vp]                   # const float* const*
    desc, plan = ctypes.POINTER(L._H.classes["srk_conv_desc"]), ctypes.POINTER(L._H.classes["srk_wgrad_plan"])
    assert P["srk_conv2d_backward_weight_plan"] == (i, [desc, i, i, i, i, plan])
    lib = L.load()
    assert lib.srk_adam_step.restype is i and list(lib.srk_adam_step.argtypes) == P["srk_adam_step"][1]


def test_callers_argument_kinds_still_pass(pkg):
    """A bare struct, byref and an array for a struct pointer; None, c_void_p, a ctypes array, data_as() and an integer
    address for every other pointer."""
    L = pkg._lib
    lib = L.load()
    d = L.ConvDesc(1, 8, 8, 3, 8, 8, 4, 3, 3, 1, 1, 0, 0, 0)
    n = lib.srk_conv2d_backward_weight_workspace_bytes(d)
    assert n > 0 and lib.srk_conv2d_backward_weight_workspace_bytes(ctypes.byref(d)) == n
    assert lib.srk_conv2d_backward_weight_workspace_bytes(ctypes.pointer(d)) == n
    phases = (L.Phase * 4)()
    phases[0].struct_size = ctypes.sizeof(L.Phase)
    assert lib.srk_trans_phases(4, 4, 2, 1, 8, 8, phases, 4) == 4 and phases[3].PH == 4
    want = np.stack([np.cos(2 * np.pi * np.arange(8) / 8), np.sin(2 * np.pi * np.arange(8) / 8)], 1)
    a = np.zeros((8, 2))
    b = (ctypes.c_double * 16)()
    for arg in (a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(a.ctypes.data),
                a.ctypes.data, b):
        a[:] = 0
        assert lib.srk_dft_table_host(8, arg) == 0
        np.testing.assert_allclose(np.frombuffer(b, np.float64).reshape(8, 2) if arg is b else a, want, atol=1e-15)
    assert lib.srk_dft_table_host(8, None) == L.ERR_BAD_ARG
    with pytest.raises(ctypes.ArgumentError):
        lib.srk_conv2d_backward_weight_workspace_bytes(L.BwdMask())      # a struct pointer stays typed


REFUSED = [
    ("unknown type", "int srk_f(foo_t x);", "foo_t.*srk_f"),
    ("unknown return type", "bar_t srk_f(int x);", "bar_t.*srk_f"),
    ("function pointer", "int srk_g(int (*cb)(int), void* stream);", "srk_g"),
    ("bit-field", "typedef struct srk_s { uint32_t a : 3; } srk_s;", "srk_s"),
    ("struct by value", "typedef struct srk_s { int32_t a; } srk_s;\nint srk_h(srk_s v);", "srk_s by value.*srk_h"),
    ("struct field by value", "typedef struct srk_s { int32_t a; } srk_s;\ntypedef struct srk_t { srk_s s; } srk_t;", "srk_t"),
    ("enumerator without =", "typedef enum srk_e { SRK_A = 0, SRK_B } srk_e;", "SRK_B.*srk_e"),
    ("nested braces", "typedef struct srk_o { struct { int32_t a; } in; } srk_o;", "srk_o"),
    ("array parameter", "int srk_k(const float x[4]);", "srk_k"),
    ("array field", "typedef struct srk_s { int32_t a[4]; } srk_s;", "srk_s"),
    ("pointer return", "float* srk_m(void);", "srk_m"),
    ("macro", "#define SRK_TWICE(x) (2 * (x))", "SRK_TWICE"),
    ("conditional", "#if SRK_FOO\nint srk_n(void);\n#endif", "SRK_FOO"),
    ("foreign name", "int other_fn(void);", "other_fn"),
]


@pytest.mark.parametrize("what,text,names", REFUSED, ids=[r[0] for r in REFUSED])
def test_reader_refuses(pkg, what, text, names):
    with pytest.raises(RuntimeError, match=names):
        pkg._header.read("#include <stdint.h>\n" + text + "\n")


def test_reader_names_a_missing_header(pkg, tmp_path):
    missing = str(tmp_path / "include" / "srk.h")
    with pytest.raises(RuntimeError, match="srk.h") as e:
        pkg._header.read_file(missing)
    assert missing in str(e.value)


def test_reader_on_a_small_header(pkg):
    h = pkg._header.read("""
        #ifndef SRK_T_H_
        #define SRK_T_H_
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define SRK_N 0x10 /* a comment */
        typedef enum srk_e { SRK_A = -1, SRK_B = SRK_A, SRK_C = 2 } srk_e;   // aliases
        enum { SRK_D = SRK_N };
        typedef struct srk_s { int32_t a, b; const float* p; uint64_t q; char name[8]; } srk_s;
        const char* srk_name(void);
        size_t srk_f(const srk_s* s, srk_s* out, const float* const* xs, long long* n, double v, void* stream);
        #ifdef __cplusplus
        }
        #endif
        #endif
        """)
    assert h.constants == {"SRK_N": 16, "SRK_A": -1, "SRK_B": -1, "SRK_C": 2, "SRK_D": 16}
    assert h.structs == {"srk_s": [("a", ctypes.c_int32), ("b", ctypes.c_int32), ("p", ctypes.c_void_p),
                                   ("q", ctypes.c_uint64), ("name", ctypes.c_char * 8)]}
    S = ctypes.POINTER(h.classes["srk_s"])
    assert h.functions == {"srk_name": (ctypes.c_char_p, []),
                           "srk_f": (ctypes.c_size_t, [S, S, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p])}
    assert h.spellings["srk_f"] == ("size_t", ["const srk_s *", "srk_s *", "const float * const *", "long long *", "double",
                                               "void *"])


def test_public_surface_keeps_names_and_values(pkg):
    L, ops = pkg._lib, pkg.ops
    assert (L.ACT_NONE, L.ACT_RELU, L.ACT_PRELU, L.ACT_LRELU, L.ACT_TANH, L.ACT_SIGMOID) == (0, 1, 2, 3, 4, 5)
    assert (L.ALGO_AUTO, L.ALGO_GENERIC, L.ALGO_MFMA, L.ALGO_DIRECT, L.ALGO_MFMA_BF16X3, L.ALGO_MFMA_BF16X6,
            L.ALGO_MFMA_F16X3) == (0, 1, 2, 3, 4, 5, 6)
    assert (L.LOSS_MSE, L.LOSS_L1, L.LOSS_CHARBONNIER, L.LOSS_BCE) == (0, 1, 2, 3)
    assert (L.VGG_TAP_POOL, L.VGG_TAP_RELU, L.VGG_TAP_LAST) == (0, 1, 2)
    assert (L.AMAX_FLOATS, L.FFT_LOSS_MAX_DIM, L.NIQE_TABLE, L.NIQE_FEATURES, L.SPECTRAL_MAX_LAYERS) == (256, 256, 9801, 36, 16)
    assert (L.ERR_UNSUPPORTED, L.ERR_BAD_ARG, L.ERR_INVALID, L.VERSION) == (-2, -1, -1, 600)
    assert L.SSIM_DOMAINS == {"float": 0, "u8": 1, "y8": 2}
    assert L.ACT_BY_NAME == {None: 0, "relu": 1, "prelu": 2, "lrelu": 3, "tanh": 4, "sigmoid": 5}
    assert ops.INTERP_BOX == 4 and ops._INTERP == {"nearest": 0, "bilinear": 2, "bicubic": 3}
    assert ops.BLUR_KINDS == {"gauss": 0, "ggauss": 1, "plateau": 2, "sinc": 3}
    assert (ops.NOISE2_OFF, ops.NOISE2_GAUSS, ops.NOISE2_POISSON) == (0, 1, 2)
    assert (ops.POISSON_KT, ops.POISSON_PEAK, ops.USM_MAX_K, ops.WATTN_MAX_HEAD_DIM) == (448, 256.0, 51, 32)
    assert ops.YUV_SUBSAMPLING == {"420": 0, "444": 1, "mono": 2}
    assert ops.JPEG_SUBSAMPLING == {"4:2:0": 1, "420": 1, 420: 1, "4:4:4": 0, "444": 0, 444: 0}
    for value in (L.ACT_NONE, L.VERSION, ops.POISSON_KT):
        assert type(value) is int


def test_constructors_behave_as_before(pkg):
    L = pkg._lib
    r = L.ConvResult()
    assert (r.struct_size, r.wrote_amax, r.bn_partial_rows) == (ctypes.sizeof(L.ConvResult), 0, 0) and r.struct_size == 12
    for cls in (L.WgradPlan, L.DenseEpilogue, L.DensePlan, L.PhaseAxis, L.Phase):
        assert cls().struct_size == ctypes.sizeof(cls) > 0
    e = L.DenseEpilogue()
    assert (e.s, e.r1, e.r2, e.ldR2, e.a1) == (1.0, 1.0, 0.0, 0, 1.0)
    e = L.DenseEpilogue(0.5, 2.0, 0.25, 48, a1=4.0)
    assert (e.struct_size, e.s, e.r1, e.r2, e.ldR2, e.a1) == (24, 0.5, 2.0, 0.25, 48, 4.0)
    d = L.ConvDesc(1, 8, 9, 3, 8, 9, 4, 3, 5, 1, 2, 0, 0, L.ALGO_MFMA)
    assert (d.N, d.H, d.W, d.Cin, d.OH, d.OW, d.Cout, d.KH, d.KW, d.stride, d.pad, d.transposed, d.out_pad, d.algo, d.x_nchw,
            d.dy_ps_r) == (1, 8, 9, 3, 8, 9, 4, 3, 5, 1, 2, 0, 0, 2, 0, 0)
    m = L.BwdMask(None, 0.2)
    assert m.y is None and abs(m.slope - 0.2) < 1e-7
    assert L.Epilogue(act=L.ACT_LRELU, slope=0.5).act == 3
    assert L.WgradPlan().name == b""


def test_load_refuses_a_library_of_another_version(pkg, monkeypatch):
    L = pkg._lib
    assert L.load().srk_version() == L.VERSION == 600
    monkeypatch.setattr(L, "VERSION", 601)          # as if the header had moved on and libsrk.so were stale
    monkeypatch.setattr(L, "_lib", None)
    with pytest.raises(RuntimeError, match="version 600 .* SRK_VERSION 601"):
        L.load()
    assert L._lib is None
