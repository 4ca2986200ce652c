"""The streaming kernels of csrc/elementwise.hip, loss_optim.hip and prepost.hip against tests/streaming_ref.py (fp64), at
the sizes where their launchers change path: below / around one float4, around one block, two or three blocks with and
without a tail, and just above each grid cap (streaming_ref.sizes).  These entry points report no kernel name
(srk_last_kernel_name is the convolutions'), so a path is selected by construction -- n % 4, pointer alignment, C % 4 --
and the docstrings say which.

Bars: conftest.assert_close_elementwise at 1e-6 for tensors, relative 1e-6 for scalar reductions, 1e-5 for the PReLU slope
gradient (float atomics); tests/test_streaming_cpu.py shows fp32 arithmetic within half of each on these inputs.

Write side: an output of a direct C-ABI call lives inside a larger tensor, NaN-filled, between two guards of 64 sentinel
floats; afterwards no NaN is left and the guards are untouched.  Every extent is checked on the host before a launch.
Read side of the reductions: mass planted at the structural positions (streaming_ref.positions).
k_sgd<4>'s 65535-block cap needs > 500 MB per buffer and is not swept.

Which test runs which kernel / branch
  k_act_fwd        float4 body, scalar tail, > 1 block, grid cap      test_act_forward_backward_sizes
                   per-channel float4 branch (C = 8, 64)              test_prelu_per_channel, test_activation_op[(3,8,4,4) / (5,12)]
                   !vec_ok scalar branch (C = 3, 6)                   test_prelu_per_channel, test_activation_op[(2,6,5,7)]
  k_act_bwd<4>     ReLU family, n % 4 == 0, aligned, grid cap         test_act_forward_backward_sizes (off = 0)
  k_act_bwd<1>     n % 4 != 0; dx off a 16-byte boundary; tanh /      test_act_forward_backward_sizes (off = 1),
                   sigmoid; per-channel slope gradient                test_prelu_per_channel
  k_axpby          body, tail, cap                                    test_axpby_sizes
  k_scale_dev      foreign upstream gradient of a loss                test_loss_seeds_and_foreign_gradients
  k_loss_partial<4> dense aligned n % 4 == 0, 1 .. 1024 blocks, cap   test_loss_sizes, test_loss_op_layouts[(2,4,6,5)]
  k_loss_partial<1> contiguous branch, cap                            test_loss_sizes, test_loss_scalar_kernel_at_multiples_of_4
                   strided branch (NCHW, crop, expand, stride 2)      test_loss_op_layouts, test_loss_scalar_kernel_at_multiples_of_4
  k_sgd<4> / <1>   first_step, lr_dev / lr, grad_scale_dev / NULL     test_sgd_sizes, test_sgd_scalar_kernel_at_multiples_of_4,
                                                                      test_clip_scale_reaches_the_scalar_sgd
  k_adam<4> / <1>  1, 2 - 3, capped blocks; the arrival ticket        test_adam_sizes, test_adam_scalar_kernel_at_multiples_of_4,
                                                                      test_tensor_adam_17
  k_sqsum_partial / k_norm_final                                      test_grad_norm_clip_sizes
  k_absmax         float4 branch, tail, unaligned branch, cap         test_absmax
  k_psnr_partial   cap, strided pred / gt                             test_psnr_sizes, test_psnr_op_layouts
  k_channel_affine cap, NHWC / NCHW channel index                     test_channel_affine_sizes, test_channel_affine_op
  k_upsample_nearest_fwd<4> / <1> / _bwd, caps                        test_upsample_op, test_upsample_above_the_caps
  k_maxpool2       odd H / W, cap                                     test_maxpool_op, test_maxpool_above_the_cap"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import streaming_ref as R
from conftest import assert_close_elementwise, rel_err  # noqa: F401
from streaming_ref import BAR, f32

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = -12345.5
NAN = float("nan")


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _lib():
    return _pkg()._lib.load()


def _sp():
    return _pkg()._lib.stream_ptr()


def _dev(a, gpu, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(dtype).to(gpu)


def _np(t):
    return t.detach().cpu().numpy()


def _p(t, elem=0):
    """device pointer of element `elem` of t (None -> NULL)"""
    if t is None:
        return None
    assert 0 <= elem < max(t.numel(), 1) and t.is_contiguous()
    return ctypes.c_void_p(t.data_ptr() + elem * t.element_size())


class Guarded(object):
    """n floats, `off` floats past a 16-byte boundary, inside one allocation with >= GUARD sentinel floats either side."""

    def __init__(self, n, gpu, off=0, init=None):
        assert n >= 1 and 0 <= off < 4
        self.n, self.lo = n, GUARD + off
        self.big = torch.full((GUARD + 4 + n + GUARD,), SENT, dtype=torch.float32, device=gpu)
        assert self.big.data_ptr() % 16 == 0 and self.lo + n + GUARD <= self.big.numel()
        self.t = self.big[self.lo:self.lo + n]
        assert self.t.data_ptr() % 16 == 4 * off and self.t.numel() == n
        if init is None:
            self.t.fill_(NAN)
        else:
            assert init.size == n
            self.t.copy_(torch.from_numpy(np.array(init, np.float32)))

    def check(self, what=""):
        """-> the payload as numpy, after: no NaN left, guards bit-identical"""
        big = _np(self.big)
        lo, hi = self.lo, self.lo + self.n
        assert (big[:lo] == np.float32(SENT)).all() and (big[hi:] == np.float32(SENT)).all(), "%s: a guard was written" % what
        assert not np.isnan(big[lo:hi]).any(), "%s: %d elements never written" % (what, int(np.isnan(big[lo:hi]).sum()))
        return big[lo:hi].copy()


def _close(got, ref, rtol, atol=None, what=""):
    """assert_close_elementwise, after: every element of `got` is finite (its `>` lets a NaN through)"""
    got = np.asarray(got)
    assert np.isfinite(got).all(), "%s: %d non-finite elements" % (what, int((~np.isfinite(got)).sum()))
    assert_close_elementwise(got, ref, rtol, atol=atol, what=what)


def _rel(got, want):
    return abs(float(got) - float(want)) / max(abs(float(want)), 1e-300)


# =====================================================================================================================
# activations
# =====================================================================================================================
def _act_fwd(gpu, x, C, kind, slope, w, off=0):
    """srk_act_forward into a guarded y -> (Guarded y, device x)"""
    n = x.size
    xd = _dev(x.reshape(-1), gpu)
    wd = _dev(w, gpu) if w is not None else None
    y = Guarded(n, gpu, off)
    assert xd.numel() == n and (w is None or w.size in (1, C)) and (w is None or w.size == 1 or n % C == 0)
    rc = _lib().srk_act_forward(_p(xd), _p(y.t), n, C, R.ACT_CODE[kind], slope, _p(wd), 0 if w is None else w.size, _sp())
    assert rc == 0, _lib().srk_last_error_string()
    return y, xd, wd


def _act_bwd(gpu, dy, saved_dev, C, kind, slope, wd, off=0):
    n = dy.size
    dyd = _dev(dy.reshape(-1), gpu)
    dx = Guarded(n, gpu, off)
    dpw = Guarded(wd.numel(), gpu, init=np.full(wd.numel(), 0.75)) if wd is not None else None
    assert saved_dev.numel() == n and dyd.numel() == n
    rc = _lib().srk_act_backward(_p(dyd), _p(saved_dev), _p(dx.t), n, C, R.ACT_CODE[kind], slope, _p(wd),
                                 0 if wd is None else wd.numel(), _p(dpw.t) if dpw else None, _sp())
    assert rc == 0, _lib().srk_last_error_string()
    return dx, dpw


ACT_SIZES = R.sizes(R.CAP_EW)


@pytest.mark.parametrize("n", ACT_SIZES)
def test_act_forward_backward_sizes(gpu, n):
    """k_act_fwd: float4 body + scalar tail (n % 4 != 0), one block .. the 4096-block cap.  Backward: k_act_bwd<4> for the ReLU
    family at n % 4 == 0, the scalar k_act_bwd<1> otherwise (and for tanh / sigmoid); with dx one float off a 16-byte boundary
    the scalar kernel at n % 4 == 0 too.  The slope gradient accumulates into a buffer that holds 0.75."""
    big = n > 10000
    x, dy = R.gen_act(n)
    slope = f32(0.2)
    for kind in (("lrelu", "prelu", "tanh") if big else ("relu", "prelu", "lrelu", "tanh", "sigmoid")):
        w = R.gen_prelu_w(1) if kind == "prelu" else None
        g = np.abs(dy) if w is not None else dy     # (one sign: the slope gradient is a sum without cancellation)
        y, xd, wd = _act_fwd(gpu, x, 1, kind, slope, w)
        yh = y.check("%s forward n=%d" % (kind, n))
        _close(yh, R.act_fwd(x, kind, slope, w), BAR, what="%s y n=%d" % (kind, n))
        saved_dev, saved = (xd, x) if w is not None else (y.t, yh)
        for off in ((0,) if big else (0, 1)):
            dx, dpw = _act_bwd(gpu, g, saved_dev, 1, kind, slope, wd, off)
            rdx, rdw = R.act_bwd(g, saved, kind, slope, w)
            _close(dx.check("%s backward" % kind), rdx, BAR, what="%s dx n=%d off=%d" % (kind, n, off))
            if w is not None:
                _close(dpw.check("dprelu"), rdw + 0.75, R.BAR_DPRELU, what="dprelu n=%d off=%d" % (n, off))


@pytest.mark.parametrize("C", [1, 3, 6, 8, 64])
@pytest.mark.parametrize("rows", [1, 5, 171, 1366])
def test_prelu_per_channel(gpu, C, rows):
    """Per-channel PReLU on [rows, C] (NHWC memory order / [B, F]): C % 4 == 0 takes the float4 body with four different
    slopes per vector, C in {3, 6} the !vec_ok scalar branch; slopes of both signs; zeros of both signs in x."""
    n = rows * C
    x, dy = R.gen_act(n, seed=C)
    dy = np.abs(dy)
    w = R.gen_prelu_w(C)
    y, xd, wd = _act_fwd(gpu, x, C, "prelu_c", 0.0, w)
    _close(y.check("prelu_c"), R.act_fwd(x.reshape(rows, C), "prelu_c", 0.0, w).reshape(-1), BAR, what="y")
    dx, dpw = _act_bwd(gpu, dy, xd, C, "prelu_c", 0.0, wd)
    rdx, rdw = R.act_bwd(dy.reshape(rows, C), x.reshape(rows, C), "prelu_c", 0.0, w)
    _close(dx.check("prelu_c dx"), rdx.reshape(-1), BAR, what="dx")
    _close(dpw.check("prelu_c dw"), rdw + 0.75, R.BAR_DPRELU, what="dw")


@pytest.mark.parametrize("kind", R.ACTS)
@pytest.mark.parametrize("shape", [(2, 6, 5, 7), (3, 8, 4, 4), (2, 1, 3, 3), (5, 12)])
def test_activation_op(gpu, kind, shape):
    """ops.activation through autograd: logical NCHW stored NHWC and [B, F]; slopes 0.0 and 0.2; torch's conventions at
    +-0 (the inputs hold both); the slope gradient lands in an existing `_srk_grad` that holds 0.75."""
    ops = _pkg().ops
    C = shape[1]
    x, dy = R.gen_act(int(np.prod(shape)), seed=sum(shape))
    x, dy = x.reshape(shape), np.abs(dy.reshape(shape))
    mem = (lambda a: a.transpose(0, 2, 3, 1)) if len(shape) == 4 else (lambda a: a)     # logical -> memory order
    for slope in ((0.0, f32(0.2)) if kind == "lrelu" else (0.0,)):
        w = {"prelu": R.gen_prelu_w(1), "prelu_c": R.gen_prelu_w(C)}.get(kind)
        xg = _dev(x, gpu).requires_grad_(True)
        wg = None
        if w is not None:
            wg = _dev(w, gpu).requires_grad_(True)
            wg._srk_grad = torch.full_like(wg, 0.75).detach()
        y = ops.activation(xg, kind.replace("prelu_c", "prelu"), slope, wg)
        yh = _np(y)
        _close(mem(yh), R.act_fwd(mem(x), kind, slope, w), BAR, what="y")
        y.backward(_dev(dy, gpu))
        rdx, rdw = R.act_bwd(mem(dy), mem(x) if w is not None else mem(yh), kind, slope, w)
        _close(mem(_np(xg.grad)), rdx, BAR, what="dx")
        if w is not None:
            assert wg.grad is None
            _close(_np(wg._srk_grad), rdw + 0.75, R.BAR_DPRELU, what="dw")
    if kind in ("relu", "lrelu", "prelu"):      # zero of either sign: relu' = 0, the slope side otherwise (torch)
        z = torch.tensor([[0.0, -0.0, 0.0, -0.0]], device=gpu, requires_grad=True)
        wz = torch.tensor([0.3], device=gpu) if kind == "prelu" else None
        ops.activation(z, kind, f32(0.2), wz).backward(torch.ones_like(z))
        want = {"relu": 0.0, "lrelu": np.float32(0.2), "prelu": np.float32(0.3)}[kind]
        assert (_np(z.grad) == want).all()


def test_lrelu_negative_slope_raises(gpu):
    """The backward decides the side by the sign of the saved output, which a negative slope flips: refused, loudly."""
    ops = _pkg().ops
    x = torch.ones(1, 4, 2, 2, device=gpu)
    with pytest.raises(RuntimeError, match="negative slope"):
        ops.activation(x, "lrelu", -0.1)
    ops.activation(x, "lrelu", 0.0)
    w = torch.tensor([-0.1], device=gpu)        # PReLU keeps x: a negative slope is fine there
    xg = -x.clone().requires_grad_(True)
    ops.activation(xg, "prelu", 0.0, w)


def test_misaligned_dense_views(gpu):
    """ops.activation / ops.add on a dense view whose storage offset is not a multiple of 16 bytes: `_dense` copies it and
    the values are right (srk_act_forward / srk_axpby themselves refuse such a pointer, with a message that says so)."""
    pkg = _pkg()
    a, b = R.gen_act(3 * 9, seed=41)
    base, other = _dev(a.reshape(3, 1, 3, 3), gpu), _dev(b.reshape(3, 1, 3, 3), gpu)
    v, u = base[1:], other[1:]
    assert v.data_ptr() % 16 != 0
    _close(_np(pkg.ops.activation(v, "tanh")), R.act_fwd(a.reshape(3, 1, 3, 3)[1:], "tanh"), BAR, what="tanh")
    assert np.array_equal(_np(pkg.ops.add(v, u)), (a + b).reshape(3, 1, 3, 3)[1:])
    flat = _dev(a, gpu)[1:]
    assert np.array_equal(_np(pkg.ops.add(flat.view(2, 13), flat.view(2, 13))), (a[1:] + a[1:]).reshape(2, 13))
    lib = _lib()
    y = Guarded(26, gpu)
    assert lib.srk_act_forward(_p(flat), _p(y.t), 26, 1, 4, 0.0, None, 0, _sp()) != 0
    assert b"aligned" in lib.srk_last_error_string()
    assert lib.srk_axpby(_p(flat), _p(flat), _p(y.t), 26, 1.0, 1.0, _sp()) != 0
    assert b"aligned" in lib.srk_last_error_string()
    torch.cuda.synchronize()
    assert np.isnan(_np(y.t)).all()


# =====================================================================================================================
# axpby
# =====================================================================================================================
@pytest.mark.parametrize("n", ACT_SIZES)
def test_axpby_sizes(gpu, n):
    """k_axpby: float4 body, scalar tail, up to the 4096-block cap; out = a + b is exact in fp32."""
    a, b = R.gen_act(n, seed=29)
    ad, bd = _dev(a, gpu), _dev(b, gpu)
    for al, be in ((1.0, 1.0), (f32(0.3), f32(-1.7))):
        out = Guarded(n, gpu)
        assert ad.numel() == n == bd.numel()
        assert _lib().srk_axpby(_p(ad), _p(bd), _p(out.t), n, al, be, _sp()) == 0
        got = out.check("axpby n=%d" % n)
        _close(got, al * a.astype(np.float64) + be * b, BAR, what="axpby n=%d" % n)
        if al == be == 1.0:
            assert np.array_equal(got, a + b)


# =====================================================================================================================
# losses
# =====================================================================================================================
LOSS_SIZES = R.sizes(R.CAP_LOSS4, R.CAP_RED)
LOSS_CODE = {k: i for i, k in enumerate(R.LOSSES)}
EPS = f32(1e-6)


def _loss_abi(gpu, kind, p, t, dims, t_dev=None, strides=None, want_grad=True, gscale=1.0):
    """srk_loss_forward_backward -> (value, dpred or None).  pred dense [N, H, W, C] memory order, flat in `p`."""
    lib = _lib()
    N, C, H, W = dims
    n = p.size
    assert n == N * C * H * W
    pd = _dev(p, gpu)
    td = t_dev if t_dev is not None else _dev(t, gpu)
    if strides is None:
        assert td.numel() == n
    else:       # the furthest element the strides reach is inside the target
        assert min(strides) >= 0 and sum((d - 1) * s for d, s in zip(dims, strides)) < td.numel()
    dp = Guarded(n, gpu) if want_grad else None
    out = Guarded(1, gpu)
    ws = torch.empty(int(lib.srk_loss_workspace_bytes()), dtype=torch.uint8, device=gpu)
    st = (ctypes.c_int64 * 4)(*strides) if strides is not None else None
    rc = lib.srk_loss_forward_backward(LOSS_CODE[kind], _p(pd), _p(td), st, N, C, H, W, EPS if kind == "charbonnier" else 0.0,
                                       gscale, _p(out.t), _p(dp.t) if dp else None, _p(ws), _sp())
    assert rc == 0, lib.srk_last_error_string()
    return float(out.check("loss")[0]), (dp.check("dpred") if dp else None)


def _check_loss(kind, p, t, where, val, g, scale=1.0, what=""):
    rv, rg = R.loss(kind, p, t, EPS)
    print("%s %s: value %.9g want %.9g (rel %.2e)" % (what, kind, val, rv, _rel(val, rv)))
    assert _rel(val, rv) <= BAR, (what, kind, val, rv)
    if g is not None:
        regular = np.ones(p.size, bool)
        regular[np.asarray(where, np.int64)] = False
        rg = rg * scale
        atol = BAR * float(np.sqrt(np.mean(rg.reshape(-1)[regular] ** 2))) if regular.any() else 0.0
        _close(g, rg, BAR, atol=atol, what="%s %s dpred" % (what, kind))


@pytest.mark.parametrize("kind", R.LOSSES)
@pytest.mark.parametrize("n", LOSS_SIZES)
def test_loss_sizes(gpu, kind, n):
    """n % 4 == 0, aligned, dense: k_loss_partial<4> (capped at 1024 blocks above 4 * 1024 * 256); otherwise k_loss_partial<1>
    (capped above 1024 * 2048).  |pred - target| is 1000 x larger at the last element, the end of the float4 body, the
    start of the second grid-stride pass and in the last block.  Without dpred the value is the same."""
    vec = n % 4 == 0
    where = R.positions(n, R.grid_loss(n, vec), 4 if vec else 1)
    p, t = R.gen_loss(kind, n, where)
    val, g = _loss_abi(gpu, kind, p, t, (1, 1, 1, n))
    _check_loss(kind, p, t, where, val, g, what="n=%d" % n)
    val2, _ = _loss_abi(gpu, kind, p, t, (1, 1, 1, n), want_grad=False)
    assert val2 == val


@pytest.mark.parametrize("kind", R.LOSSES)
@pytest.mark.parametrize("n", [4, 1024, 4096, R.CAP_RED + 4])
def test_loss_scalar_kernel_at_multiples_of_4(gpu, kind, n):
    """A dense target one float off a 16-byte boundary: the scalar kernel at n % 4 == 0, contiguous branch; and the same
    target through explicit strides with a stride-2 W (the strided branch)."""
    where = R.positions(n, R.grid_red(n))
    p, t = R.gen_loss(kind, n, where)
    tg = Guarded(n, gpu, off=1, init=t)
    val, g = _loss_abi(gpu, kind, p, t, (1, 1, 1, n), t_dev=tg.t, gscale=f32(0.25))
    _check_loss(kind, p, t, where, val, g, scale=f32(0.25), what="misaligned n=%d" % n)
    if n <= 4096:
        t2 = torch.zeros(2 * n, device=gpu)
        t2[::2] = _dev(t, gpu)
        val, g = _loss_abi(gpu, kind, p, t, (1, 1, 1, n), t_dev=t2, strides=(2 * n, 1, 2 * n, 2))
        _check_loss(kind, p, t, where, val, g, what="strided n=%d" % n)


def _target_cases(gpu, t, shape):
    """(name, device tensor of the logical values t) in the layouts a loader or a view can hand over"""
    N, C, H, W = shape
    td = _dev(t, gpu)
    yield "nchw", td
    yield "channels_last", td.contiguous(memory_format=torch.channels_last)
    big = torch.full((N, C, H + 3, W + 5), NAN, device=gpu)
    big[:, :, 1:1 + H, 2:2 + W] = td
    yield "crop", big[:, :, 1:1 + H, 2:2 + W]
    bigcl = torch.full((N + 1, C, H, W), NAN, device=gpu).contiguous(memory_format=torch.channels_last)
    bigcl[1:] = td
    yield "batch_slice", bigcl[1:]


@pytest.mark.parametrize("kind", R.LOSSES)
@pytest.mark.parametrize("shape", [(2, 3, 9, 11), (2, 4, 6, 5), (2, 1, 9, 11), (1, 3, 9, 11), (2, 3, 1, 11), (2, 3, 9, 1)])
def test_loss_op_layouts(gpu, kind, shape):
    """ops.*_loss with pred NCHW / channels_last against targets that are NCHW, channels_last, a spatial crop, a batch
    slice (misaligned for odd C H W) or expanded over the batch; size-1 dims, where torch reports arbitrary strides.
    (2, 3, 9, 11) is 594 elements (scalar kernel), (2, 4, 6, 5) is 240 (the float4 kernel for a channels_last target)."""
    ops = _pkg().ops
    fn = {"mse": ops.mse_loss, "l1": ops.l1_loss, "charbonnier": lambda a, b: ops.charbonnier_loss(a, b, EPS),
          "bce": ops.bce_loss}[kind]
    n = int(np.prod(shape))
    p, t = R.gen_loss(kind, n, (0, n - 1, n // 4 * 4 - 1))
    p, t = p.reshape(shape), t.reshape(shape)
    rv, rg = R.loss(kind, p, t, EPS)
    regular = np.ones(n, bool)
    regular[[0, n - 1, n // 4 * 4 - 1]] = False
    atol = BAR * float(np.sqrt(np.mean(rg.reshape(-1)[regular] ** 2)))
    for pred_cl in (False, True):
        for name, td in _target_cases(gpu, t, shape):
            pg = _dev(p, gpu)
            if pred_cl:
                pg = pg.contiguous(memory_format=torch.channels_last)
            pg.requires_grad_(True)
            l = fn(pg, td)
            assert _rel(l.item(), rv) <= BAR, (name, pred_cl, l.item(), rv)
            ops.backward(l)                      # the unit seed: the stored gradient as it is
            _close(_np(pg.grad), rg, BAR, atol=atol, what="%s %s" % (kind, name))
    # a target expanded over the batch (stride 0)
    te = t[:1]
    pg = _dev(p, gpu).requires_grad_(True)
    l = fn(pg, _dev(te, gpu).expand(*shape))
    rv, rg = R.loss(kind, p, np.broadcast_to(te, shape), EPS)
    assert _rel(l.item(), rv) <= BAR
    ops.backward(l)
    _close(_np(pg.grad), rg, BAR, what="%s expand" % kind)


@pytest.mark.parametrize("kind", R.LOSSES)
def test_loss_seeds_and_foreign_gradients(gpu, kind):
    """No grad: the value alone.  Under ops.loss_seed(v, t) the stored gradient is v * dL/dpred; any other upstream gradient
    -- autograd's own ones of loss.backward(), a weight -- goes through k_scale_dev and is right too."""
    ops = _pkg().ops
    fn = {"mse": ops.mse_loss, "l1": ops.l1_loss, "charbonnier": lambda a, b: ops.charbonnier_loss(a, b, EPS),
          "bce": ops.bce_loss}[kind]
    shape = (2, 3, 9, 11)
    p, t = R.gen_loss(kind, 594)
    p, t = p.reshape(shape), t.reshape(shape)
    rv, rg = R.loss(kind, p, t, EPS)
    td = _dev(t, gpu)
    with torch.no_grad():
        assert _rel(fn(_dev(p, gpu), td).item(), rv) <= BAR
    seed = torch.full((), 0.25, device=gpu)
    for mode, factor in (("plain", 1.0), ("weight", 2.5), ("seeded", 0.25), ("seeded_foreign", 3.0)):
        pg = _dev(p, gpu).requires_grad_(True)
        if mode.startswith("seeded"):
            with ops.loss_seed(0.25, seed):
                l = fn(pg, td)
        else:
            l = fn(pg, td)
        assert _rel(l.item(), rv) <= BAR
        if mode == "plain":
            l.backward()
        elif mode == "seeded":
            ops.backward(l, seed)
        else:
            l.backward(torch.full((), factor, device=gpu))
        _close(_np(pg.grad), rg * factor, BAR, what="%s %s" % (kind, mode))


def test_bce_clamps_and_rows(gpu):
    """pred exactly 0.0 and 1.0 against targets 0 and 1: log clamped at -100, the gradient's denominator at 1e-12; [B, 1]
    (the discriminator's output).  Pure relative bar: the 1e12-class gradients must not lend the others an allowance."""
    ops = _pkg().ops
    p, t = R.gen_loss("bce", 12)
    p[:4], t[:4] = (0.0, 0.0, 1.0, 1.0), (0.0, 1.0, 0.0, 1.0)
    for shape in ((12, 1), (3, 4), (1, 1, 3, 4)):
        pg = _dev(p.reshape(shape), gpu).requires_grad_(True)
        l = ops.bce_loss(pg, _dev(t.reshape(shape), gpu))
        rv, rg = R.loss("bce", p, t)
        assert _rel(l.item(), rv) <= BAR
        ops.backward(l)
        _close(_np(pg.grad).reshape(-1), rg, BAR, atol=0.0, what="bce %s" % (shape,))


# =====================================================================================================================
# SGD / Adam / clip, direct ABI
# =====================================================================================================================
OPT_SIZES = R.sizes(R.CAP_RED)
# which of {lr as an argument | lr_dev} x {grad_scale_dev NULL | 0.25} a variant's sweep uses: all four are covered
SGD_MODES = {"plain": (False, None), "momentum": (True, 0.25), "momentum_wd": (False, 0.25), "nesterov": (True, None)}


def _sgd_run(gpu, n, variant, off):
    lib = _lib()
    hp = R.SGD_VARIANTS[variant]
    lr_on_dev, gs = SGD_MODES[variant]
    p0, grads = R.gen_opt(n)
    p = Guarded(n, gpu, off, init=p0)
    buf = Guarded(n, gpu, off) if hp["mom"] else None      # NaN-filled: first_step = 1 must not read it
    lr_dev = torch.tensor([R.SGD_LR], device=gpu) if lr_on_dev else None
    gs_dev = torch.tensor([gs], device=gpu) if gs is not None else None
    gds = [Guarded(n, gpu, off, init=g) for g in grads]
    for k, gd in enumerate(gds):
        assert p.t.numel() == n == gd.t.numel() and (buf is None or buf.t.numel() == n)
        rc = lib.srk_sgd_step(_p(p.t), _p(gd.t), _p(buf.t) if buf else None, n, 0.0 if lr_on_dev else R.SGD_LR, hp["mom"],
                              hp["wd"], int(hp["nesterov"]), int(k == 0), _p(lr_dev), _p(gs_dev), _sp())
        assert rc == 0, lib.srk_last_error_string()
    rp, rbuf = R.run_sgd(p0, grads, variant, gs if gs is not None else 1.0)
    what = "sgd %s n=%d off=%d" % (variant, n, off)
    _close(p.check(what), rp, BAR, what=what + " p")
    if buf:
        _close(buf.check(what + " buffer"), rbuf, BAR, what=what + " buf")
    for gd, g in zip(gds, grads):
        assert np.array_equal(gd.check(what), g)


@pytest.mark.parametrize("variant", sorted(R.SGD_VARIANTS))
@pytest.mark.parametrize("n", OPT_SIZES)
def test_sgd_sizes(gpu, variant, n):
    """Three chained steps, the first with first_step = 1 over a NaN-filled momentum buffer.  n % 4 == 0: k_sgd<4>; otherwise
    k_sgd<1> (capped at 1024 blocks above 1024 * 2048)."""
    _sgd_run(gpu, n, variant, 0)


@pytest.mark.parametrize("variant", sorted(R.SGD_VARIANTS))
@pytest.mark.parametrize("n", [8, 4096])
def test_sgd_scalar_kernel_at_multiples_of_4(gpu, variant, n):
    """buffers one float off a 16-byte boundary: k_sgd<1> at n % 4 == 0"""
    _sgd_run(gpu, n, variant, 1)


def _adam_run(gpu, n, wd, off):
    lib = _lib()
    lr_on_dev, gs = (False, None) if wd == 0.0 else (True, 0.25)
    p0, grads = R.gen_opt(n)
    z = np.zeros(n, np.float32)
    p, m, v = Guarded(n, gpu, off, init=p0), Guarded(n, gpu, off, init=z), Guarded(n, gpu, off, init=z)
    stepbig = torch.full((GUARD + 2 + GUARD,), -77, dtype=torch.int32, device=gpu)
    step = stepbig[GUARD:GUARD + 2]
    step.zero_()
    lr_dev = torch.tensor([R.ADAM["lr"]], device=gpu) if lr_on_dev else None
    gs_dev = torch.tensor([gs], device=gpu) if gs is not None else None
    gds = [_dev(g, gpu) for g in grads]
    for gd in gds:       # back to back on the stream: every launch reads the count the previous one left
        assert gd.numel() == n and gd.data_ptr() % 16 == 0
        rc = lib.srk_adam_step(_p(p.t), _p(gd), _p(m.t), _p(v.t), n, 0.0 if lr_on_dev else R.ADAM["lr"], R.ADAM["b1"],
                               R.ADAM["b2"], R.ADAM["eps"], wd, _p(step), _p(lr_dev), _p(gs_dev), _sp())
        assert rc == 0, lib.srk_last_error_string()
    what = "adam n=%d wd=%g off=%d" % (n, wd, off)
    sb = _np(stepbig)
    assert sb[GUARD:GUARD + 2].tolist() == [len(grads), 0], what
    assert (sb[:GUARD] == -77).all() and (sb[GUARD + 2:] == -77).all()
    rp, rm, rv, _ = R.run_adam(p0, grads, wd, gs if gs is not None else 1.0)
    _close(p.check(what), rp, BAR, what=what + " p")
    _close(m.check(what), rm, BAR, what=what + " m")
    _close(v.check(what), rv, BAR, what=what + " v")


@pytest.mark.parametrize("wd", [0.0, f32(1e-4)])
@pytest.mark.parametrize("n", R.sizes(R.CAP_ADAM4, R.CAP_RED))
def test_adam_sizes(gpu, wd, n):
    """Three steps launched back to back; afterwards {count, ticket} = [3, 0].  n % 4 == 0: k_adam<4> (1, 2 - 3 and, above
    4 * 512 * 512, the capped 2 * CUs blocks); otherwise k_adam<1> (capped above 1024 * 2048).  lr 0.05: the three steps move p
    by 0.1 - 0.3 of |p|, so an error of the step is not hidden by p's own rounding."""
    _adam_run(gpu, n, wd, 0)


@pytest.mark.parametrize("n", [8, 4096])
def test_adam_scalar_kernel_at_multiples_of_4(gpu, n):
    _adam_run(gpu, n, f32(1e-4), 1)


def test_tensor_adam_17(gpu):
    """optim.TensorAdam on 17 elements (DRCN's combine weights): the scalar k_adam<1>, one block, lr on the device."""
    pkg = _pkg()
    p0, grads = R.gen_opt(17)
    t = _dev(p0, gpu)
    opt = pkg.optim.TensorAdam(t, R.ADAM["lr"], betas=(R.ADAM["b1"], R.ADAM["b2"]), eps=R.ADAM["eps"])
    for g in grads:
        opt.grad.copy_(_dev(g, gpu))
        opt.step()
    rp, rm, rv, _ = R.run_adam(p0, grads)
    assert opt.step_dev.tolist() == [3, 0]
    _close(_np(t), rp, BAR, what="p")
    _close(_np(opt.exp_avg), rm, BAR, what="m")
    _close(_np(opt.exp_avg_sq), rv, BAR, what="v")


def _norm_abi(gpu, gd, n, max_norm):
    lib = _lib()
    out = Guarded(2, gpu)
    ws = torch.empty(int(lib.srk_grad_norm_workspace_bytes()), dtype=torch.uint8, device=gpu)
    assert gd.numel() == n
    assert lib.srk_grad_norm_clip(_p(gd), n, max_norm, _p(out.t, 0), _p(out.t, 1), _p(ws), _sp()) == 0
    return out


@pytest.mark.parametrize("n", OPT_SIZES)
def test_grad_norm_clip_sizes(gpu, n):
    """k_sqsum_partial up to its 1024-block cap, +-1 planted among 1e-3-class gradients at the structural positions; the
    scale on both sides of max_norm."""
    where = R.positions(n, R.grid_red(n))
    g = R.gen_mass(n, where)
    gd = _dev(g, gpu)
    norm = R.clip(g, 1.0)[0]
    for max_norm in (f32(0.5 * norm), f32(2.0 * norm)):
        got = _norm_abi(gpu, gd, n, max_norm).check("norm")
        rn, rs = R.clip(g, max_norm)
        print("n=%d norm %.9g want %.9g scale %.9g want %.9g" % (n, got[0], rn, got[1], rs))
        assert _rel(got[0], rn) <= BAR and _rel(got[1], rs) <= BAR
        assert (got[1] == 1.0) == (max_norm > rn)


def test_clip_scale_reaches_the_scalar_sgd(gpu):
    """the scale srk_grad_norm_clip leaves on the device is what the next (scalar, n % 4 == 3) SGD step multiplies by"""
    lib = _lib()
    n = 4099
    g = R.gen_mass(n, R.positions(n, R.grid_red(n)))
    p0, _ = R.gen_opt(n)
    gd = _dev(g, gpu)
    out = _norm_abi(gpu, gd, n, 0.4)
    p = Guarded(n, gpu, init=p0)
    assert lib.srk_sgd_step(_p(p.t), _p(gd), None, n, 1.0, 0.0, 0.0, 0, 0, None, _p(out.t, 1), _sp()) == 0
    scale = R.clip(g, f32(0.4))[1]
    assert scale < 1.0
    _close(p.check("sgd"), R.sgd_step(p0, g, None, 1.0, gs=scale)[0], BAR, what="clipped step")


# =====================================================================================================================
# absmax
# =====================================================================================================================
@pytest.mark.parametrize("n", R.sizes(R.CAP_ABSMAX))
def test_absmax(gpu, n):
    """The maximum, positive and negative, planted at each structural position of the float4 branch and of the scalar one;
    the pointer on a 16-byte boundary and 4, 8, 12 bytes past it (k_absmax's unaligned branch).  Exact."""
    lib = _lib()
    AM = _pkg()._lib.AMAX_FLOATS
    blocks = R.grid_absmax(n)
    where = sorted(set(R.positions(n, blocks, 4) + R.positions(n, blocks, 1)))
    x = (R._rs(n % 1000).uniform(-0.5, 0.5, n)).astype(np.float32)
    base = torch.zeros(n + 4, device=gpu)
    slots = Guarded(AM, gpu)
    results, wants = [], []
    for k in ((0, 1, 2, 3) if n < 10000 else (0, 1)):
        xd = base[k:k + n]
        assert k + n <= base.numel() and xd.data_ptr() % 16 == 4 * k
        xd.copy_(torch.from_numpy(x))
        for i in [None] + where:
            for v in ((3.0, -3.0) if i is not None else (None,)):
                if i is not None:
                    xd[i] = v
                slots.t.zero_()
                assert lib.srk_absmax(_p(xd), n, _p(slots.t), _sp()) == 0
                results.append(slots.t.max().reshape(1))
                wants.append(3.0 if i is not None else R.absmax(x))
            if i is not None:
                xd[i] = float(x[i])
    slots.check("absmax slots")
    assert _np(torch.cat(results)).tolist() == wants


# =====================================================================================================================
# PSNR
# =====================================================================================================================
def _psnr_abi(gpu, pd, ps, gd, gs, dims):
    lib = _lib()
    out = Guarded(2, gpu)
    ws = torch.empty(int(lib.srk_psnr_workspace_bytes()), dtype=torch.uint8, device=gpu)
    N, C, H, W = dims
    for t, s in ((pd, ps), (gd, gs)):      # the furthest element either stride set reaches is inside its tensor
        assert (N - 1) * s[0] + (C - 1) * s[1] + (H - 1) * s[2] + (W - 1) * s[3] < t.numel() and min(s) >= 0
    rc = lib.srk_psnr(_p(pd), (ctypes.c_int64 * 4)(*ps), _p(gd), (ctypes.c_int64 * 4)(*gs), N, C, H, W, _p(out.t, 0),
                      _p(out.t, 1), _p(ws), _sp())
    assert rc == 0
    return out.check("psnr")


@pytest.mark.parametrize("n", OPT_SIZES)
def test_psnr_sizes(gpu, n):
    """k_psnr_partial up to its 1024-block cap; the difference is 1000 x larger at the structural positions."""
    where = R.positions(n, R.grid_red(n))
    gt = R._rs(7).uniform(0.25, 0.75, n).astype(np.float32)
    pred = gt + R.gen_mass(n, where) * np.float32(0.25)
    got = _psnr_abi(gpu, _dev(pred, gpu), (n, 1, n, 1), _dev(gt, gpu), (n, 1, n, 1), (1, 1, 1, n))
    rp, rm = R.psnr(pred, gt)
    print("n=%d mse %.9g want %.9g psnr %.9g want %.9g" % (n, got[1], rm, got[0], rp))
    assert _rel(got[1], rm) <= BAR and _rel(got[0], rp) <= BAR


def test_psnr_op_layouts(gpu):
    """ops.psnr: identical inputs give 100; pred outside [0, 1] is clamped; channels_last pred against an NCHW gt; crops of
    both; [C, H, W]."""
    ops = _pkg().ops
    shape = (2, 3, 9, 11)
    gt = R._rs(1).uniform(size=shape).astype(np.float32)
    pred = (gt + R._rs(2).uniform(-0.3, 0.3, size=shape)).astype(np.float32)     # leaves [0, 1] on both sides
    assert pred.min() < 0 and pred.max() > 1
    gd, pd = _dev(gt, gpu), _dev(pred, gpu)
    ps, mse = ops.psnr(gd, gd.clone())
    assert ps.item() == 100.0 and mse.item() == 0.0
    rp, rm = R.psnr(pred, gt)
    bigp = torch.full((2, 3, 12, 16), NAN, device=gpu)
    bigp[:, :, 2:11, 3:14] = pd
    bigg = torch.full((2, 3, 10, 13), NAN, device=gpu).contiguous(memory_format=torch.channels_last)
    bigg[:, :, 1:10, 0:11] = gd
    for a, b in ((pd, gd), (pd.contiguous(memory_format=torch.channels_last), gd), (bigp[:, :, 2:11, 3:14], bigg[:, :, 1:10, 0:11])):
        ps, mse = ops.psnr(a, b)
        assert _rel(mse.item(), rm) <= BAR and _rel(ps.item(), rp) <= BAR
    rp, rm = R.psnr(pred[0], gt[0])
    ps, mse = ops.psnr(pd[0], gd[0])
    assert _rel(mse.item(), rm) <= BAR and _rel(ps.item(), rp) <= BAR


# =====================================================================================================================
# channel affine, nearest up-sampling, 2x2 max-pool
# =====================================================================================================================
SUB, DIV = (0.4, 0.5, 0.6, 0.1, 0.2, 0.3, 0.7, 0.8), (0.2, 0.25, 0.3, 0.9, 1.1, 0.6, 0.45, 2.0)


@pytest.mark.parametrize("n", R.sizes(R.CAP_PP))
def test_channel_affine_sizes(gpu, n):
    """k_channel_affine up to its 4096-block cap, flat: channel = (e / inner) % C for NHWC (inner 1) and NCHW-like
    (inner 5) storage; bit-equal to fp32 (x - sub) / div."""
    lib = _lib()
    x = R._rs(3).standard_normal(n).astype(np.float32)
    xd = _dev(x, gpu)
    for C, inner, clamp in ((3, 1, 0), (3, 5, 1)):
        y = Guarded(n, gpu)
        fa, fb = (ctypes.c_float * C)(*SUB[:C]), (ctypes.c_float * C)(*DIV[:C])
        assert xd.numel() == n
        assert lib.srk_channel_affine(_p(xd), _p(y.t), n, C, inner, fa, fb, clamp, _sp()) == 0
        c = (np.arange(n) // inner) % C
        want = (x - np.asarray(SUB, np.float32)[c]) / np.asarray(DIV, np.float32)[c]
        if clamp:
            want = np.clip(want, np.float32(0), np.float32(1))
        assert np.array_equal(y.check("channel_affine"), want)


@pytest.mark.parametrize("C", [1, 3, 8])
def test_channel_affine_op(gpu, C):
    """ops.channel_affine, NCHW / channels_last / [C, H, W], clamped or not: torch.equal to x.sub(m).div(s) in torch fp32;
    the backward is dy / div."""
    ops = _pkg().ops
    x = R._rs(C).standard_normal((2, C, 5, 7)).astype(np.float32)
    xt = torch.from_numpy(x)
    m, s = torch.tensor(SUB[:C]).view(1, C, 1, 1), torch.tensor(DIV[:C]).view(1, C, 1, 1)
    want = xt.sub(m).div(s)
    for xd in (xt.to(gpu), xt.to(gpu).contiguous(memory_format=torch.channels_last)):
        assert torch.equal(ops.channel_affine(xd, SUB, DIV).cpu(), want)
        assert torch.equal(ops.channel_affine(xd, SUB, DIV, clamp01=True).cpu(), want.clamp(0, 1))
        xg = xd.clone().requires_grad_(True)
        dy = R._rs(9).standard_normal((2, C, 5, 7)).astype(np.float32)
        ops.channel_affine(xg, SUB, DIV).backward(_dev(dy, gpu))
        _close(_np(xg.grad), R.channel_affine(dy, [0.0] * C, [f32(v) for v in DIV]), BAR, what="dx")
    assert torch.equal(ops.channel_affine(xt[0].to(gpu), SUB, DIV).cpu(), want[0])


@pytest.mark.parametrize("r", [2, 3, 4])
def test_upsample_op(gpu, r):
    """ops.upsample_nearest: C % 4 == 0 takes the float4 kernel, the rest the scalar one; odd H / W.  Forward bit-equal to
    F.interpolate(mode="nearest"), backward against the fp64 block sums."""
    ops = _pkg().ops
    for C in (1, 3, 4, 6, 64):
        x = R._rs(C + r).standard_normal((2, C, 5, 7)).astype(np.float32)
        xg = _dev(x, gpu).requires_grad_(True)
        y = ops.upsample_nearest(xg, r)
        assert torch.equal(y.detach().cpu(), F.interpolate(torch.from_numpy(x), scale_factor=r, mode="nearest")), (r, C)
        dy = R._rs(C).standard_normal((2, C, 5 * r, 7 * r)).astype(np.float32)
        y.backward(_dev(dy, gpu))
        _close(_np(xg.grad), R.upsample_bwd(dy, r), BAR, what="upsample dx r=%d C=%d" % (r, C))


@pytest.mark.parametrize("C,H,W", [(4, 1025, 512), (3, 592, 592)])
def test_upsample_above_the_caps(gpu, C, H, W):
    """r = 2, direct ABI into guarded outputs: the float4 kernel above 4 * 4096 * 512 outputs, the scalar one above
    4096 * 1024; the backward above its 4096 blocks of 512 inputs."""
    lib = _lib()
    r = 2
    nin, nout = H * W * C, H * r * W * r * C
    assert nout > (R.CAP_UP4 if C % 4 == 0 else R.CAP_PP)
    x = R._rs(C).standard_normal((1, H, W, C)).astype(np.float32)          # memory order
    xd = _dev(x.reshape(-1), gpu)
    y = Guarded(nout, gpu)
    assert xd.numel() == nin
    assert lib.srk_upsample_nearest_forward(_p(xd), _p(y.t), 1, H, W, C, r, _sp()) == 0
    want = np.repeat(np.repeat(x, r, axis=1), r, axis=2)
    assert np.array_equal(y.check("upsample").reshape(want.shape), want)
    dy = R._rs(C + 1).standard_normal((1, H * r, W * r, C)).astype(np.float32)
    dyd = _dev(dy.reshape(-1), gpu)
    dx = Guarded(nin, gpu)
    assert dyd.numel() == nout
    assert lib.srk_upsample_nearest_backward(_p(dyd), _p(dx.t), 1, H, W, C, r, _sp()) == 0
    ref = dy.astype(np.float64).reshape(1, H, r, W, r, C).sum(axis=(2, 4))
    _close(dx.check("upsample dx").reshape(ref.shape), ref, BAR, what="dx")


@pytest.mark.parametrize("C", [1, 3, 64])
def test_maxpool_op(gpu, C):
    """ops.max_pool2x2, floor mode: odd H and / or W drop the trailing row / column; H == 2, W == 2."""
    ops = _pkg().ops
    for H, W in ((5, 7), (6, 6), (7, 8), (2, 9), (9, 2), (2, 2), (3, 3)):
        x = R._rs(H * W + C).standard_normal((2, C, H, W)).astype(np.float32)
        want = F.max_pool2d(torch.from_numpy(x), 2, 2)
        assert np.array_equal(want.numpy(), R.maxpool2(x))
        for xd in (_dev(x, gpu), _dev(x, gpu).contiguous(memory_format=torch.channels_last)):
            with torch.no_grad():
                assert torch.equal(ops.max_pool2x2(xd).cpu(), want), (C, H, W)


def test_maxpool_above_the_cap(gpu):
    """more than 4096 * 1024 outputs, odd H and W, into a guarded output"""
    lib = _lib()
    C, H, W = 3, 2 * 1367 + 1, 2 * 1024 + 1
    nout = 1367 * 1024 * C
    assert nout > R.CAP_PP
    x = R._rs(5).standard_normal((1, H, W, C)).astype(np.float32)
    xd = _dev(x.reshape(-1), gpu)
    y = Guarded(nout, gpu)
    assert xd.numel() == H * W * C
    assert lib.srk_maxpool2x2_forward(_p(xd), _p(y.t), 1, H, W, C, _sp()) == 0
    want = x[:, :H - 1, :W - 1].reshape(1, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))
    assert np.array_equal(y.check("maxpool").reshape(want.shape), want)
