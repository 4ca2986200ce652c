"""The channel-slice convolution on the GPU (ops.dense_conv / dense_conv_backward_data / dense_conv_backward_weight over
csrc/dense.hip) against the fp64 restatement of tests/rdn_ref.py, case by case over rdn_ref.CASES: sources and
destinations are slices at non-zero channel offsets of wider buffers.

For every case: forward, data gradient and weight gradient against fp64; every byte of a destination buffer outside the
slice keeps its bits; the channels around the source slices are NaN and the results finite (they are never read); beta 0
overwrites a NaN-filled destination and beta 1 adds; two calls give the same bits; the device agrees with the host twin.

Bars: outputs within 1e-4, gradients within 1e-3 of max |fp64 reference|, every element."""
import ctypes

import pytest
import torch

import rdn_ref as R

pytestmark = pytest.mark.gpu

TOL_FWD, TOL_GRAD = 1e-4, 1e-3


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _bits_equal(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _host(pkg, d, direction, **kw):
    lib = pkg._lib.load()
    p = lambda v: v if (v is None or isinstance(v, ctypes.c_void_p)) else R.fptr(v)
    g = lambda k: p(kw.get(k))
    rc = lib.srk_dense_conv_host(ctypes.byref(d), direction, g("A"), g("B"), g("W"), g("bias"), g("res"), g("y"), g("dy"),
                                 g("add"), g("dA"), kw.get("betaA", 0.0), g("dB"), kw.get("betaB", 0.0), g("dW"), g("db"),
                                 kw.get("beta", 0.0))
    assert rc == 0, lib.srk_last_error_string().decode()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_forward(gpu, name):
    pkg, c = _pkg(), R.case(name)
    ops = pkg.ops
    n, h, w = c.dims
    Y = c.out_buf(c.cout, 32, c.cout + 48)
    a, b = c.A.device(gpu), (c.B.device(gpu) if c.B else None)
    res = c.R.device(gpu) if c.R else None
    wt, bias = c.W.to(gpu), c.bias.to(gpu)

    def run():
        out = Y.device(gpu).clone(memory_format=torch.preserve_format)
        got = ops.dense_conv(a, wt, bias, b, out, c.ca, c.A.off, c.cb, c.B.off if c.B else 0, Y.off, c.act, R.SLOPE, res,
                             c.R.off if c.R else 0, c.terms)
        assert got is out
        return R.from_device(out)

    first, second = run(), run()
    got = first[..., Y.off:Y.off + c.cout].permute(0, 3, 1, 2)
    assert bool(torch.isfinite(got).all())                      # NaN all around the source slices: never read
    err = R.worst(got, c.y)
    print("dense fwd %s terms %d: worst %.3e of max |ref|" % (name, c.terms, err))
    assert err <= TOL_FWD
    assert Y.outside_equal(first)                               # nothing outside the destination slice moved
    assert _bits_equal(first, second)
    # the host twin, same addressing
    H = c.out_buf(c.cout, 32, c.cout + 48)
    d = R.desc(pkg, n, h, w, c.k, c.ca, c.cb, c.cout, c.act, R.SLOPE, c.terms, ldA=c.A.width, ldB=c.B.width if c.B else 0,
               ldY=H.width, ldR=c.R.width if c.R else 0)
    _host(pkg, d, 0, A=c.A.ptr(), B=c.B.ptr() if c.B else None, W=c.W, bias=c.bias, res=c.R.ptr() if c.R else None, y=H.ptr())
    assert R.worst(got, H.nchw()) <= TOL_FWD


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward_data(gpu, name):
    pkg, c = _pkg(), R.case(name)
    ops = pkg.ops
    n, h, w = c.dims
    DA, DB = c.out_buf(c.ca, 16, c.ca + 32), (c.out_buf(c.cb, 48, c.cb + 64) if c.cb else None)
    dy, ys, add, wt = c.DY.device(gpu), c.YS.device(gpu), c.ADD.device(gpu), c.W.to(gpu)
    with_act = c.act != R.ACT_NONE

    def run(da, db, beta, with_add):
        ops.dense_conv_backward_data(dy, wt, c.ca, c.cb, ys if with_act else None, da, db, add if with_add else None,
                                     c.DY.off, c.YS.off, DA.off, DB.off if DB else 0, c.ADD.off, beta, beta, c.act, R.SLOPE,
                                     c.terms)

    fresh = lambda B_: B_.device(gpu).clone(memory_format=torch.preserve_format) if B_ else None
    da, db = fresh(DA), fresh(DB)
    run(da, db, 0.0, True)                                      # beta 0 over NaN-filled slices, the skip's gradient added
    da2, db2 = fresh(DA), fresh(DB)
    run(da2, db2, 0.0, True)
    assert _bits_equal(da, da2) and (db is None or _bits_equal(db, db2))
    got_a = R.from_device(da)
    sl_a = got_a[..., DA.off:DA.off + c.ca].permute(0, 3, 1, 2)
    want_a = c.da + c.ADD.nchw().double()
    assert bool(torch.isfinite(sl_a).all()) and DA.outside_equal(got_a)
    err_a = R.worst(sl_a, want_a)
    err_b = 0.0
    if DB:
        got_b = R.from_device(db)
        sl_b = got_b[..., DB.off:DB.off + c.cb].permute(0, 3, 1, 2)
        assert bool(torch.isfinite(sl_b).all()) and DB.outside_equal(got_b)
        err_b = R.worst(sl_b, c.db)
    print("dense dgrad %s terms %d: worst dA %.3e, dB %.3e of max |ref|" % (name, c.terms, err_a, err_b))
    assert err_a <= TOL_GRAD and err_b <= TOL_GRAD
    # the host twin
    HA, HB = c.out_buf(c.ca, 16, c.ca + 32), (c.out_buf(c.cb, 48, c.cb + 64) if c.cb else None)
    d = R.desc(pkg, n, h, w, c.k, c.ca, c.cb, c.cout, c.act, R.SLOPE, c.terms, ldDy=c.DY.width, ldY=c.YS.width,
               ldDA=HA.width, ldDB=HB.width if HB else 0, ldAdd=c.ADD.width)
    _host(pkg, d, 1, W=c.W, y=c.YS.ptr(), dy=c.DY.ptr(), add=c.ADD.ptr(), dA=HA.ptr(), dB=HB.ptr() if HB else None)
    assert R.worst(sl_a, HA.nchw()) <= TOL_GRAD and (not DB or R.worst(sl_b, HB.nchw()) <= TOL_GRAD)
    # beta 1 adds to what is there, without the skip this time
    run(da, db, 1.0, False)
    got_a = R.from_device(da)
    assert R.worst(got_a[..., DA.off:DA.off + c.ca].permute(0, 3, 1, 2), want_a + c.da) <= TOL_GRAD
    assert DA.outside_equal(got_a)
    if DB:
        got_b = R.from_device(db)
        assert R.worst(got_b[..., DB.off:DB.off + c.cb].permute(0, 3, 1, 2), 2 * c.db) <= TOL_GRAD
        assert DB.outside_equal(got_b)
        # one destination alone
        only_b = fresh(DB)
        ops.dense_conv_backward_data(dy, wt, c.ca, c.cb, ys if with_act else None, None, only_b, None, c.DY.off, c.YS.off, 0,
                                     DB.off, 0, 0.0, 0.0, c.act, R.SLOPE, c.terms)
        assert _bits_equal(only_b, db2)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward_weight(gpu, name):
    pkg, c = _pkg(), R.case(name)
    ops = pkg.ops
    n, h, w = c.dims
    a, b = c.A.device(gpu), (c.B.device(gpu) if c.B else None)
    dy, ys = c.DY.device(gpu), c.YS.device(gpu)
    with_act = c.act != R.ACT_NONE

    def run(dw, dbias, beta):
        ops.dense_conv_backward_weight(a, dy, dw, dbias, b, ys if with_act else None, c.ca, c.A.off, c.cb,
                                       c.B.off if c.B else 0, c.DY.off, c.YS.off, beta, c.act, R.SLOPE, c.terms)

    # the gradients live inside one flat buffer, as a parameter's do: its neighbours must not move
    nw, nb = c.W.numel(), c.bias.numel()
    flat = torch.arange(nw + nb + 64, dtype=torch.float32, device=gpu) + 0.25
    before = flat.clone()
    dw, dbias = flat[16:16 + nw].view(c.W.shape), flat[32 + nw:32 + nw + nb]
    dw.fill_(float("nan"))
    dbias.fill_(float("nan"))
    run(dw, dbias, 0.0)                                         # beta 0 over NaN
    first_w, first_b = dw.clone(), dbias.clone()
    assert bool(torch.isfinite(first_w).all()) and bool(torch.isfinite(first_b).all())
    assert torch.equal(flat[:16], before[:16]) and torch.equal(flat[16 + nw:32 + nw], before[16 + nw:32 + nw])
    assert torch.equal(flat[32 + nw + nb:], before[32 + nw + nb:])
    err_w, err_b = R.worst(first_w, c.dw), R.worst(first_b, c.dbias)
    print("dense wgrad %s terms %d: worst dW %.3e, db %.3e of max |ref|" % (name, c.terms, err_w, err_b))
    assert err_w <= TOL_GRAD and err_b <= TOL_GRAD
    dw2, db2 = torch.full_like(first_w, float("nan")), torch.full_like(first_b, float("nan"))
    run(dw2, db2, 0.0)
    assert _bits_equal(first_w, dw2) and _bits_equal(first_b, db2)
    run(dw, dbias, 1.0)                                         # beta 1 adds
    assert R.worst(dw, 2 * c.dw) <= TOL_GRAD and R.worst(dbias, 2 * c.dbias) <= TOL_GRAD
    # the host twin
    hw_, hb_ = torch.full_like(c.W, float("nan")), torch.full_like(c.bias, float("nan"))
    d = R.desc(pkg, n, h, w, c.k, c.ca, c.cb, c.cout, c.act, R.SLOPE, c.terms, ldA=c.A.width, ldB=c.B.width if c.B else 0,
               ldDy=c.DY.width, ldY=c.YS.width)
    _host(pkg, d, 2, A=c.A.ptr(), B=c.B.ptr() if c.B else None, y=c.YS.ptr(), dy=c.DY.ptr(), dW=hw_, db=hb_)
    assert R.worst(first_w, hw_) <= TOL_GRAD and R.worst(first_b, hb_) <= TOL_GRAD


def test_unsupported_is_a_value_error_that_names_the_number(gpu):
    ops = _pkg().ops
    x = torch.zeros(1, 24, 4, 4, device=gpu).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="CA = 24"):
        ops.dense_conv(x, torch.zeros(16, 24, 3, 3, device=gpu))
    x = torch.zeros(1, 32, 4, 4, device=gpu).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="Cout = 80"):
        ops.dense_conv(x, torch.zeros(80, 32, 3, 3, device=gpu))
    with pytest.raises(ValueError, match="K = 5"):
        ops.dense_conv(x, torch.zeros(16, 32, 5, 5, device=gpu))
    with pytest.raises(ValueError, match="CB = 8"):
        ops.dense_conv(x, torch.zeros(16, 24, 3, 3, device=gpu), b=x, ca=16, cb=8)
    with pytest.raises(ValueError, match=r"\[16, 56\)"):
        ops.dense_conv(x, torch.zeros(16, 40, 3, 3, device=gpu), ca=40, a_off=16)
    with pytest.raises(ValueError, match="pointer is not 16-byte aligned"):
        ops.dense_conv(x, torch.zeros(16, 16, 3, 3, device=gpu), ca=16, a_off=2)
