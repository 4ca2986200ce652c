"""The channel-slice convolution without a GPU: the host twin (srk_dense_conv_host) against the fp64 restatement of
tests/rdn_ref.py on sliced buffers -- strides, offsets, both betas, the order of [A | B] -- the refusals, the exported
symbols and the planner."""
import ctypes

import pytest
import torch

import rdn_ref as R

TOL_FWD, TOL_GRAD = 1e-4, 1e-3


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _pkg()._lib.load()


def _host(lib, d, direction, A=None, B=None, W=None, bias=None, res=None, y=None, dy=None, add=None, dA=None, betaA=0.0,
          dB=None, betaB=0.0, dW=None, db=None, beta=0.0):
    p = lambda v: v if (v is None or isinstance(v, ctypes.c_void_p)) else R.fptr(v)
    return lib.srk_dense_conv_host(ctypes.byref(d), direction, p(A), p(B), p(W), p(bias), p(res), p(y), p(dy), p(add), p(dA),
                                   betaA, p(dB), betaB, p(dW), p(db), beta)


def _desc(c, **ld):
    n, h, w = c.dims
    return R.desc(_pkg(), n, h, w, c.k, c.ca, c.cb, c.cout, c.act, R.SLOPE, c.terms, **ld)


@pytest.mark.parametrize("name", R.SMALL_CASES)
def test_host_twin_matches_the_restatement(lib, name):
    c = R.case(name)
    # forward into a NaN-filled slice of a patterned buffer
    Y = c.out_buf(c.cout, 32, c.cout + 48)
    before = Y.t.clone()
    d = _desc(c, ldA=c.A.width, ldB=c.B.width if c.B else 0, ldY=Y.width, ldR=c.R.width if c.R else 0)
    assert _host(lib, d, 0, A=c.A.ptr(), B=c.B.ptr() if c.B else None, W=c.W, bias=c.bias, res=c.R.ptr() if c.R else None,
                 y=Y.ptr()) == 0
    assert R.worst(Y.nchw(), c.y) <= 1e-6 and Y.outside_equal(before)          # fp64 accumulation, one rounding
    # data gradient: beta 0 over NaN with `add`, then beta 1 on top of it
    DA, DB = c.out_buf(c.ca, 16, c.ca + 32), (c.out_buf(c.cb, 48, c.cb + 64) if c.cb else None)
    before_a, before_b = DA.t.clone(), (DB.t.clone() if DB else None)
    d = _desc(c, ldDy=c.DY.width, ldY=c.YS.width, ldDA=DA.width, ldDB=DB.width if DB else 0, ldAdd=c.ADD.width)
    args = dict(W=c.W, y=c.YS.ptr(), dy=c.DY.ptr(), dA=DA.ptr(), dB=DB.ptr() if DB else None)
    assert _host(lib, d, 1, add=c.ADD.ptr(), betaA=0.0, betaB=0.0, **args) == 0
    assert R.worst(DA.nchw(), c.da + c.ADD.nchw().double()) <= 1e-6 and DA.outside_equal(before_a)
    if DB:
        assert R.worst(DB.nchw(), c.db) <= 1e-6 and DB.outside_equal(before_b)
    assert _host(lib, d, 1, betaA=1.0, betaB=1.0, **args) == 0
    assert R.worst(DA.nchw(), 2 * c.da + c.ADD.nchw().double()) <= 1e-6 and DA.outside_equal(before_a)
    if DB:
        assert R.worst(DB.nchw(), 2 * c.db) <= 1e-6 and DB.outside_equal(before_b)
    # weight gradient: beta 0 over NaN, then beta 1
    dW, db = torch.full_like(c.W, float("nan")), torch.full_like(c.bias, float("nan"))
    d = _desc(c, ldA=c.A.width, ldB=c.B.width if c.B else 0, ldDy=c.DY.width, ldY=c.YS.width)
    args = dict(A=c.A.ptr(), B=c.B.ptr() if c.B else None, y=c.YS.ptr(), dy=c.DY.ptr(), dW=dW, db=db)
    assert _host(lib, d, 2, beta=0.0, **args) == 0
    assert R.worst(dW, c.dw) <= 1e-6 and R.worst(db, c.dbias) <= 1e-6
    assert _host(lib, d, 2, beta=1.0, **args) == 0
    assert R.worst(dW, 2 * c.dw) <= 1e-6 and R.worst(db, 2 * c.dbias) <= 1e-6


def test_order_of_the_two_sources(lib):
    """[A | B] is torch.cat((A, B), 1): swapping the sources without swapping the weight's halves changes the result."""
    c = R.case("1x1_k3_two")
    Y = c.out_buf(c.cout, 0, c.cout)
    d = _desc(c, ldA=c.B.width, ldB=c.A.width, ldY=Y.width)
    d.CA, d.CB = c.cb, c.ca
    assert _host(lib, d, 0, A=c.B.ptr(), B=c.A.ptr(), W=c.W, bias=c.bias, y=Y.ptr()) == 0
    want = R.conv_forward(c.B.nchw(), c.A.nchw(), c.W, c.bias, c.act)
    assert R.worst(Y.nchw(), want) <= 1e-6
    assert R.worst(Y.nchw(), c.y_act) > 1e-2


def test_block_restatement_matches_the_fp32_cat_composition():
    """rdb_forward in double is the plain fp32 torch.cat + conv2d block up to fp32 rounding."""
    blocks = R.make_blocks(16, 16, 3, 2, 7)
    x = R.rand((2, 16, 7, 9), 5)
    got = R.trunk_forward(x, blocks)
    want = R.trunk_forward(x.double(), [tuple(p.double() for p in b) for b in blocks])
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 32, 7, 9)
    assert R.worst(got, want) <= 1e-5
    one = R.rdb_forward(x.double(), [p.double() for p in blocks[0]])
    assert torch.equal(want[:, :16], one)


def test_the_slice_scheme_of_the_trunk_is_the_restatement(lib):
    """The addressing ops.residual_dense_blocks uses, run through the host twin: per block one growth buffer, layer c reading
    A = the block input and B = growth[.., :(c - 1) G] and writing growth[.., (c - 1) G : c G] with ReLU, the 1x1 fusion
    reading [A | growth], adding A and writing slice d of the fusion buffer, which block d + 1 reads in place -- no cat
    anywhere, and the fusion buffer is cat(RDB_1 .. RDB_D) of the restatement."""
    g0, g, C, D = 16, 32, 3, 2
    n, h, w = 2, 5, 7
    blocks = R.make_blocks(g0, g, C, D, 9)
    x = R.rand((n, g0, h, w), 4)
    want = R.trunk_forward(x.double(), [tuple(p.double() for p in b) for b in blocks])
    xin = x.permute(0, 2, 3, 1).contiguous()
    fusion = torch.full((n, h, w, D * g0), float("nan"))
    off = lambda t, c: ctypes.c_void_p(t.data_ptr() + 4 * c)
    for d, p in enumerate(blocks):
        growth = torch.full((n, h, w, C * g), float("nan"))
        a, lda = (off(xin, 0), g0) if d == 0 else (off(fusion, (d - 1) * g0), D * g0)
        for c in range(C):
            dd = R.desc(_pkg(), n, h, w, 3, g0, c * g, g, R.ACT_RELU, ldA=lda, ldB=C * g, ldY=C * g)
            assert _host(lib, dd, 0, A=a, B=off(growth, 0) if c else None, W=p[2 * c], bias=p[2 * c + 1],
                         y=off(growth, c * g)) == 0
        dd = R.desc(_pkg(), n, h, w, 1, g0, C * g, g0, R.ACT_NONE, ldA=lda, ldB=C * g, ldY=D * g0, ldR=lda)
        assert _host(lib, dd, 0, A=a, B=off(growth, 0), W=p[2 * C], bias=p[2 * C + 1], res=a, y=off(fusion, d * g0)) == 0
    assert R.worst(fusion.permute(0, 3, 1, 2), want) <= 1e-6


@pytest.mark.parametrize("field,value,status", [("CA", 24, -2), ("CB", 8, -2), ("Cout", 80, -2), ("Cout", 20, -2),
                                                ("K", 5, -2), ("terms", 4, -1), ("act", 4, -1), ("N", 0, -1)])
def test_refusals_name_the_number(lib, field, value, status):
    d = R.desc(_pkg(), 1, 4, 4, 3, 16, 16, 16, ldA=16, ldB=16, ldY=16)
    setattr(d, field, value)
    one = torch.zeros(4)
    assert lib.srk_dense_conv_supported(ctypes.byref(d)) == 0
    assert _host(lib, d, 0, A=one, B=one, W=one, bias=one, y=one) == status      # refused before anything is read
    msg = lib.srk_last_error_string().decode()
    assert field in msg and str(value) in msg, msg
    assert lib.srk_dense_conv_workspace_bytes(ctypes.byref(d)) == 0


def test_strides_are_checked(lib):
    one = torch.zeros(4)
    d = R.desc(_pkg(), 1, 4, 4, 3, 16, 0, 16, ldA=12, ldY=16)
    assert lib.srk_dense_conv_supported(ctypes.byref(d)) == 0
    assert _host(lib, d, 0, A=one, W=one, y=one) == -1 and "ldA = 12" in lib.srk_last_error_string().decode()
    d.ldA, d.ldY = 16, 18
    assert _host(lib, d, 0, A=one, W=one, y=one) == -2 and "ldY = 18" in lib.srk_last_error_string().decode()
    d.ldY = 16
    assert lib.srk_dense_conv_supported(ctypes.byref(d)) == 1
    assert _host(lib, d, 1, W=one, dy=one, dA=one, betaA=0.5) == -1          # a beta that is neither 0 nor 1


def test_symbols_are_declared_and_exported(lib):
    L = _pkg()._lib
    names = ["srk_dense_conv_%s" % s for s in ("supported", "plan", "workspace_bytes", "forward", "backward_data",
                                               "backward_weight", "host")]
    declared = L.header_symbols()
    for n in names:
        assert n in declared and n in L._PROTOTYPES and hasattr(lib, n), n
    assert lib.srk_version() == 600
    ops = _pkg().ops
    for n in ("dense_conv", "dense_conv_backward_data", "dense_conv_backward_weight", "residual_dense_blocks", "dense_terms"):
        assert callable(getattr(ops, n)), n


def test_terms_follow_the_precision_mode():
    ops = _pkg().ops
    before = ops.get_precision()
    try:
        want = {"mixed": (6, 6, 3), "bf16x6": (6, 6, 3), "faithful": (6, 6, 6), "bf16x3": (3, 3, 3), "fp32": (6, 6, 6)}
        for mode, terms in want.items():
            ops.set_precision(mode)
            assert tuple(ops.dense_terms(r) for r in ("infer", "train_fwd", "bwd")) == terms, mode
    finally:
        ops.set_precision(before)


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 1, 1), (2, 3, 5), (2, 17, 33), (16, 32, 32), (16, 48, 48), (2, 129, 128),
                                  (2, 181, 183), (1, 1024, 1024)])
@pytest.mark.parametrize("k,ca,cb,cout", [(1, 16, 0, 16), (3, 64, 0, 64), (3, 64, 448, 64), (1, 64, 512, 64), (3, 16, 48, 48)])
def test_planner(lib, dims, k, ca, cb, cout):
    """The workspace holds every range's partials, the ranges cover every pixel and none is empty, and a wave's pixel
    tiles are 1, 2 or 4."""
    L = _pkg()._lib
    n, h, w = dims
    d = R.desc(_pkg(), n, h, w, k, ca, cb, cout)
    plan = L.DensePlan()
    assert lib.srk_dense_conv_plan(ctypes.byref(d), ctypes.byref(plan)) == 0
    P = n * h * w
    assert plan.partial_floats == cout * (ca + cb) * k * k + cout
    assert plan.splits >= 1 and plan.split_pixels % 32 == 0
    assert plan.splits * plan.split_pixels >= P > (plan.splits - 1) * plan.split_pixels
    assert plan.ws_bytes >= plan.splits * plan.partial_floats * 4
    assert plan.ws_bytes == lib.srk_dense_conv_workspace_bytes(ctypes.byref(d)) <= 64 << 20
    assert plan.pix_tiles in (1, 2, 4)
    assert plan.pix_tiles == (4 if P // 64 >= 1024 else 2 if P // 32 >= 1024 else 1)
