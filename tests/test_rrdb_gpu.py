"""The RRDB on the GPU: the slice convolution with a scaled output and two scaled skips (the _ex entry points of
csrc/dense.hip through ops.dense_conv / dense_conv_backward_data / dense_conv_backward_weight) and ops.rrdb_trunk against
the fp64 restatement of tests/esrgan_ref.py.

The operators: (F, G) in {(16, 16), (64, 32)} -- the second gives conv5 192 input channels, across the 32-channel staging
chunks -- at N x H x W in {1x5x7, 2x17x19} (pixel counts that are no multiple of 16 or 64), 3 and 6 terms, in the two
shapes an RRDB launches: conv5 (F + 4G -> F, no activation, the RRDB epilogue) and a growth convolution (F + 2G -> G,
LeakyReLU, an epilogue with every scale odd).  Sources and destinations are slices at non-zero channel offsets of wider
buffers; everything outside a destination slice keeps its bits.

The trunk, for 1 and 2 RRDBs: output, dx and every parameter gradient; 15 launches an RRDB forward and no other launch;
repeated and graph-replayed calls give the eager call's bits.

Bars: outputs within 1e-4, gradients within 1e-3 of max |fp64 reference|, every element."""
import pytest
import torch

import esrgan_ref as E
import rdn_ref as R

pytestmark = pytest.mark.gpu

TOL_FWD, TOL_GRAD = 1e-4, 1e-3
DIMS = {"1x5x7": (1, 5, 7), "2x17x19": (2, 17, 19)}
_MADE = {}


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _bits_equal(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


class _Case(object):
    """Buffers and fp64 results of one operator case; built once, nobody writes into its members."""

    def __init__(self, f, g, dims, kind):
        n, h, w = DIMS[dims]
        self.dims = (n, h, w)
        if kind == "conv5":
            self.ca, self.cb, self.cout, self.act, self.epi = f, 4 * g, f, R.ACT_NONE, E.EPILOGUES["rrdb"]
        else:
            self.ca, self.cb, self.cout, self.act, self.epi = f, 2 * g, g, R.ACT_LRELU, E.EPILOGUES["all_odd"]
        ca, cb, cout = self.ca, self.cb, self.cout
        seed = 7000 + f + 3 * g + 11 * n + (0 if kind == "conv5" else 500)
        self.A = R.Buf(n, h, w, ca, off=16, width=ca + 48, seed=seed)
        self.B = R.Buf(n, h, w, cb, off=32, width=cb + 48, seed=seed + 1)
        self.W = R.rand((cout, ca + cb, 3, 3), seed + 2, (2.0 / ((ca + cb) * 9)) ** 0.5)
        self.bias = R.rand((cout,), seed + 3, 0.1)
        self.R1 = R.Buf(n, h, w, cout, off=16, width=cout + 16, seed=seed + 4)
        self.R2 = R.Buf(n, h, w, cout, off=32, width=cout + 48, seed=seed + 7)
        self.DY = R.Buf(n, h, w, cout, off=48, width=cout + 64, seed=seed + 5)
        self.ADD = R.Buf(n, h, w, ca, off=16, width=ca + 32, seed=seed + 6)
        s, r1, _, r2, _, a1 = self.epi
        a, b = self.A.nchw(), self.B.nchw()
        self.y_act, da, db, dw, dbias = R.conv_grads(a, b, self.W, self.bias, self.DY.nchw(), self.act, E.SLOPE)
        self.y = s * self.y_act + r1 * self.R1.nchw().double() + r2 * self.R2.nchw().double()
        self.da, self.db, self.dw, self.dbias = s * da + a1 * self.ADD.nchw().double(), s * db, s * dw, s * dbias
        self.da_plain = s * da
        self.YS = R.Buf(n, h, w, cout, off=16, width=cout + 32, inside=self.y_act.permute(0, 2, 3, 1).float())

    def out_buf(self, c, off, width):
        n, h, w = self.dims
        b = R.Buf(n, h, w, c, off=off, width=width, outside=0.0, inside=float("nan"))
        pattern = torch.arange(b.t.numel(), dtype=torch.float32).view(b.t.shape) * 0.5 + 1.0
        keep = b.t[..., off:off + c].clone()
        b.t.copy_(pattern)
        b.t[..., off:off + c] = keep
        return b


def _case(f, g, dims, kind):
    key = (f, g, dims, kind)
    if key not in _MADE:
        _MADE[key] = _Case(*key)
    return _MADE[key]


@pytest.mark.parametrize("terms", [3, 6])
@pytest.mark.parametrize("kind", ["conv5", "growth"])
@pytest.mark.parametrize("dims", sorted(DIMS))
@pytest.mark.parametrize("fg", [(16, 16), (64, 32)], ids=["F16_G16", "F64_G32"])
def test_ex_operators(gpu, fg, dims, kind, terms):
    ops = _pkg().ops
    c = _case(fg[0], fg[1], dims, kind)
    s, r1, _, r2, _, a1 = c.epi
    a, b, wt, bias = c.A.device(gpu), c.B.device(gpu), c.W.to(gpu), c.bias.to(gpu)
    dy, ys, add = c.DY.device(gpu), c.YS.device(gpu), c.ADD.device(gpu)
    with_act = c.act != R.ACT_NONE
    fresh = lambda buf: buf.device(gpu).clone(memory_format=torch.preserve_format)
    tag = "%s F%d G%d %s terms %d" % (kind, fg[0], fg[1], dims, terms)

    # forward
    Y = c.out_buf(c.cout, 32, c.cout + 48)

    def fwd():
        out = fresh(Y)
        got = ops.dense_conv(a, wt, bias, b, out, c.ca, c.A.off, c.cb, c.B.off, Y.off, c.act, E.SLOPE, c.R1.device(gpu),
                             c.R1.off, terms, s=s, r1=r1, residual2=c.R2.device(gpu), res2_off=c.R2.off, r2=r2)
        assert got is out
        return R.from_device(out)

    first, second = fwd(), fwd()
    got = first[..., Y.off:Y.off + c.cout].permute(0, 3, 1, 2)
    assert bool(torch.isfinite(got).all())                      # NaN all around the source slices: never read
    err = R.worst(got, c.y)
    print("ex fwd %s: worst %.3e of max |ref|" % (tag, err))
    assert err <= TOL_FWD
    assert Y.outside_equal(first) and _bits_equal(first, second)

    # data gradient: beta 0 over NaN with the scaled add, then beta 1 without it
    DA, DB = c.out_buf(c.ca, 16, c.ca + 32), c.out_buf(c.cb, 48, c.cb + 64)

    def dgrad(da, db, beta, with_add):
        ops.dense_conv_backward_data(dy, wt, c.ca, c.cb, ys if with_act else None, da, db, add if with_add else None,
                                     c.DY.off, c.YS.off, DA.off, DB.off, c.ADD.off, beta, beta, c.act, E.SLOPE, terms, s=s,
                                     a1=a1)

    da, db = fresh(DA), fresh(DB)
    dgrad(da, db, 0.0, True)
    da2, db2 = fresh(DA), fresh(DB)
    dgrad(da2, db2, 0.0, True)
    assert _bits_equal(da, da2) and _bits_equal(db, db2)
    got_a, got_b = R.from_device(da), R.from_device(db)
    sl_a = got_a[..., DA.off:DA.off + c.ca].permute(0, 3, 1, 2)
    sl_b = got_b[..., DB.off:DB.off + c.cb].permute(0, 3, 1, 2)
    assert bool(torch.isfinite(sl_a).all()) and bool(torch.isfinite(sl_b).all())
    assert DA.outside_equal(got_a) and DB.outside_equal(got_b)
    err_a, err_b = R.worst(sl_a, c.da), R.worst(sl_b, c.db)
    print("ex dgrad %s: worst dA %.3e, dB %.3e of max |ref|" % (tag, err_a, err_b))
    assert err_a <= TOL_GRAD and err_b <= TOL_GRAD
    dgrad(da, db, 1.0, False)
    got_a, got_b = R.from_device(da), R.from_device(db)
    assert R.worst(got_a[..., DA.off:DA.off + c.ca].permute(0, 3, 1, 2), c.da + c.da_plain) <= TOL_GRAD
    assert R.worst(got_b[..., DB.off:DB.off + c.cb].permute(0, 3, 1, 2), 2 * c.db) <= TOL_GRAD
    assert DA.outside_equal(got_a) and DB.outside_equal(got_b)

    # weight gradient, inside one flat buffer as a parameter's lives: beta 0 over NaN, then beta 1
    nw, nb = c.W.numel(), c.bias.numel()
    flat = torch.arange(nw + nb + 64, dtype=torch.float32, device=gpu) + 0.25
    before = flat.clone()
    dw, dbias = flat[16:16 + nw].view(c.W.shape), flat[32 + nw:32 + nw + nb]

    def wgrad(dw_, db_, beta):
        ops.dense_conv_backward_weight(a, dy, dw_, db_, b, ys if with_act else None, c.ca, c.A.off, c.cb, c.B.off, c.DY.off,
                                       c.YS.off, beta, c.act, E.SLOPE, terms, s=s)

    dw.fill_(float("nan"))
    dbias.fill_(float("nan"))
    wgrad(dw, dbias, 0.0)
    first_w, first_b = dw.clone(), dbias.clone()
    assert bool(torch.isfinite(first_w).all()) and bool(torch.isfinite(first_b).all())
    assert torch.equal(flat[:16], before[:16]) and torch.equal(flat[16 + nw:32 + nw], before[16 + nw:32 + nw])
    assert torch.equal(flat[32 + nw + nb:], before[32 + nw + nb:])
    err_w, err_bias = R.worst(first_w, c.dw), R.worst(first_b, c.dbias)
    print("ex wgrad %s: worst dW %.3e, db %.3e of max |ref|" % (tag, err_w, err_bias))
    assert err_w <= TOL_GRAD and err_bias <= TOL_GRAD
    dw2, db2_ = torch.full_like(first_w, float("nan")), torch.full_like(first_b, float("nan"))
    wgrad(dw2, db2_, 0.0)
    assert _bits_equal(first_w, dw2) and _bits_equal(first_b, db2_)
    wgrad(dw, dbias, 1.0)
    assert R.worst(dw, 2 * c.dw) <= TOL_GRAD and R.worst(dbias, 2 * c.dbias) <= TOL_GRAD


@pytest.mark.parametrize("terms", [3, 6])
@pytest.mark.parametrize("name", ["7x9_lrelu_res", "17x33_single_res", "7x9_k1_lff", "181x183_four_tiles"])
def test_identity_epilogue_gives_the_bits_of_the_plain_entry_points(gpu, name, terms):
    """s = r1 = a1 = 1 without R2: the _ex kernels are the plain ones bit for bit, all three directions (cases of
    tests/rdn_ref.py, the last one at four pixel tiles a wave)."""
    ops = _pkg().ops
    c = R.case(name)
    a, b = c.A.device(gpu), (c.B.device(gpu) if c.B else None)
    wt, bias, res = c.W.to(gpu), c.bias.to(gpu), c.R.device(gpu)
    dy, ys, add = c.DY.device(gpu), c.YS.device(gpu), c.ADD.device(gpu)
    with_act = c.act != R.ACT_NONE
    boff = c.B.off if c.B else 0
    fresh = lambda buf: buf.device(gpu).clone(memory_format=torch.preserve_format)
    Y = c.out_buf(c.cout, 32, c.cout + 48)
    outs = []
    for ex in (None, 1.0):
        y = fresh(Y)
        ops.dense_conv(a, wt, bias, b, y, c.ca, c.A.off, c.cb, boff, Y.off, c.act, R.SLOPE, res, c.R.off, terms, s=ex)
        DA, DB = c.out_buf(c.ca, 16, c.ca + 32, inside=0.5), (c.out_buf(c.cb, 48, c.cb + 64) if c.cb else None)
        da, db = fresh(DA), (fresh(DB) if DB else None)
        ops.dense_conv_backward_data(dy, wt, c.ca, c.cb, ys if with_act else None, da, db, add, c.DY.off, c.YS.off, DA.off,
                                     DB.off if DB else 0, c.ADD.off, 1.0, 0.0, c.act, R.SLOPE, terms, s=ex)
        dw, dbias = torch.full_like(wt, float("nan")), torch.full_like(bias, float("nan"))
        ops.dense_conv_backward_weight(a, dy, dw, dbias, b, ys if with_act else None, c.ca, c.A.off, c.cb, boff, c.DY.off,
                                       c.YS.off, 0.0, c.act, R.SLOPE, terms, s=ex)
        outs.append((y, da, db if db is not None else dw, dw, dbias))
    for p, q in zip(*outs):
        assert _bits_equal(p, q)
    assert R.worst(R.from_device(outs[1][0])[..., Y.off:Y.off + c.cout].permute(0, 3, 1, 2), c.y) <= TOL_FWD


def _trunk_inputs(f, g, nb, shape, gpu):
    blocks = E.make_blocks(f, g, nb, 40 + f)
    x = R.rand((2, f) + shape, 3)
    gy = R.rand((2, f) + shape, 4)
    return blocks, x, gy


@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("fg", [(16, 16), (64, 32)], ids=["F16_G16", "F64_G32"])
def test_trunk_matches_fp64(gpu, fg, nb, monkeypatch):
    f, g = fg
    pkg = _pkg()
    ops = pkg.ops
    shape = (7, 9)
    blocks, x, gy = _trunk_inputs(f, g, nb, shape, gpu)
    x64 = x.double().requires_grad_(True)
    b64 = E.to64(blocks, True)
    want = E.trunk_forward(x64, b64)
    want.backward(gy.double())

    # every launch of the op goes through one of these three (one launch each; the weight gradient: two)
    calls = {"fwd": 0, "dgrad": 0, "wgrad": 0}
    real = (ops.dense_conv, ops.dense_conv_backward_data, ops.dense_conv_backward_weight)

    def counted(key, fn):
        def run(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return run

    monkeypatch.setattr(ops, "dense_conv", counted("fwd", real[0]))
    monkeypatch.setattr(ops, "dense_conv_backward_data", counted("dgrad", real[1]))
    monkeypatch.setattr(ops, "dense_conv_backward_weight", counted("wgrad", real[2]))

    def forbidden(*a, **k):
        raise AssertionError("an elementwise launch or a concatenation inside ops.rrdb_trunk")

    gyd = gy.to(gpu).contiguous(memory_format=torch.channels_last)

    def run():
        xd = x.to(gpu).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        bd = [tuple(tuple(t.to(gpu).requires_grad_(True) for t in p) for p in b) for b in blocks]
        with monkeypatch.context() as m:
            for name in ("_axpby", "activation", "add"):
                m.setattr(ops, name, forbidden)
            m.setattr(torch, "cat", forbidden)
            out = ops.rrdb_trunk(xd, bd, E.RES_SCALE)
            counts_fwd = dict(calls)
            out.backward(gyd)
        return xd, bd, out, counts_fwd

    xd, bd, got, counts_fwd = run()
    assert counts_fwd == {"fwd": 15 * nb, "dgrad": 0, "wgrad": 0}
    assert calls == {"fwd": 15 * nb, "dgrad": 15 * nb, "wgrad": 15 * nb}
    assert tuple(got.shape) == (2, f) + shape and got.is_contiguous(memory_format=torch.channels_last)
    err = R.worst(got.detach(), want.detach())
    print("rrdb trunk F%d G%d nb %d forward: worst %.3e of max |ref|" % (f, g, nb, err))
    assert err <= TOL_FWD
    e = R.worst(xd.grad, x64.grad)
    worst = ("dx", e)
    assert e <= TOL_GRAD
    for i in range(nb):
        for k in range(3):
            for j, (p, q) in enumerate(zip(bd[i][k], b64[i][k])):
                assert p.grad is not None and p.grad.shape == p.shape, (i, k, j)
                e = R.worst(p.grad, q.grad)
                worst = max(worst, ("rrdb %d rdb %d param %d" % (i, k + 1, j), e), key=lambda v: v[1])
                assert e <= TOL_GRAD, (i, k, j, e)
    print("rrdb trunk F%d G%d nb %d gradients: worst %.3e of max |ref| (%s)" % (f, g, nb, worst[1], worst[0]))
    # two calls, the same bits
    xd2, bd2, got2, _ = run()
    assert torch.equal(got2, got) and torch.equal(xd2.grad, xd.grad)
    assert all(torch.equal(p.grad, q.grad) for b, c in zip(bd, bd2) for r, s in zip(b, c) for p, q in zip(r, s))
    # an input that needs no gradient: one data-gradient launch fewer, the same parameter gradients
    for key in calls:
        calls[key] = 0
    bd3 = [tuple(tuple(t.detach().clone().requires_grad_(True) for t in p) for p in b) for b in bd]
    ops.rrdb_trunk(x.to(gpu), bd3, E.RES_SCALE).backward(gyd)
    assert calls == {"fwd": 15 * nb, "dgrad": 15 * nb - 1, "wgrad": 15 * nb}
    assert all(torch.equal(p.grad, q.grad) for b, c in zip(bd, bd3) for r, s in zip(b, c) for p, q in zip(r, s))


@pytest.mark.parametrize("how", ["no_grad_on_trainable_parameters", "nothing_requires_grad"])
def test_a_forward_without_a_backward_keeps_one_growth_buffer(gpu, how, monkeypatch):
    """test() and test_single run the TRAINING model under torch.no_grad(): the op must take the inference path -- one
    growth buffer and three trunk maps however many blocks, nothing saved, no graph -- and give the training forward's
    output where the two run the same term count."""
    ops = _pkg().ops
    f, g, nb = 16, 16, 3
    made = {"growth": 0, "trunk": 0}
    real_g, real_t = ops._growth_buffer, ops._trunk_buffer
    monkeypatch.setattr(ops, "_growth_buffer", lambda *a: made.__setitem__("growth", made["growth"] + 1) or real_g(*a))
    monkeypatch.setattr(ops, "_trunk_buffer", lambda *a: made.__setitem__("trunk", made["trunk"] + 1) or real_t(*a))
    trainable = how == "no_grad_on_trainable_parameters"
    blocks = [tuple(tuple(t.to(gpu).requires_grad_(trainable) for t in p) for p in b) for b in E.make_blocks(f, g, nb, 7)]
    x = R.rand((2, f, 7, 9), 3).to(gpu).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        out = ops.rrdb_trunk(x, blocks)
    assert made == {"growth": 1, "trunk": 3} and out.grad_fn is None and not out.requires_grad
    want = E.trunk_forward(x.cpu().double(), E.to64(blocks))
    assert R.worst(out, want) <= TOL_FWD
    if trainable:
        made.update(growth=0, trunk=0)
        kept = ops.rrdb_trunk(x, blocks)
        assert made == {"growth": 3 * nb, "trunk": 3 * nb} and kept.grad_fn is not None
        assert R.worst(kept.detach(), want) <= TOL_FWD


@pytest.mark.parametrize("nb", [1, 2])
def test_replayed_graph_equals_eager(gpu, nb):
    pkg = _pkg()
    ops = pkg.ops
    f, g = 32, 16
    blocks, x, gy = _trunk_inputs(f, g, nb, (6, 5), gpu)
    bd = [tuple(tuple(t.to(gpu).requires_grad_(True) for t in p) for p in b) for b in blocks]
    params = [t for b in bd for p in b for t in p]
    xg = x.to(gpu).contiguous(memory_format=torch.channels_last)
    gyg = gy.to(gpu).contiguous(memory_format=torch.channels_last)

    def fn(x_in, gy_in):
        for p in params:
            p.grad = None
        xi = x_in.detach().requires_grad_(True)
        out = ops.rrdb_trunk(xi, bd, E.RES_SCALE)
        out.backward(gy_in)
        return [out.detach(), xi.grad] + [p.grad for p in params]

    eager = [t.clone() for t in fn(xg, gyg)]
    graph = pkg.trainers.capture_step(fn, [xg, gyg], warmup=0)
    graph(torch.ones_like(xg), gyg)                      # another batch in between
    got = [t.clone() for t in graph(xg, gyg)]
    graph.close()
    assert len(got) == 2 + 30 * nb
    for i, (a, b) in enumerate(zip(eager, got)):
        assert torch.equal(a, b), i
