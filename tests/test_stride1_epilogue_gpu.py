"""Stride-1 convolutions and their data gradients: every kernel family, every fused epilogue and every store path, on
guarded outputs against float64 (through the C ABI: srk_conv2d_forward_ex, srk_conv2d_backward_data, srk_conv2d_backward_data_relu,
srk_pack_weight_fwd / _bwd with the row's ps_r).

The rows are the table of tests/stride1_epilogue_ref.py (CASES; its FAMILIES says what each family's predicate accepts and
what makes it decline, tests/test_stride1_epilogue_cpu.py checks that every such pair has a row and that every row's inputs
make a pass meaningful).  A row states the kernel it expects; one that reaches another kernel fails.

Inputs: oracle.fill.randn, the outermost two rows and columns of x and dy times 4; NHWC tensors (NCHW for x_nchw rows) cut
from one flat allocation at a 16-byte boundary or the row's byte offset past one; the output NaN-filled between sentinel
guards.  The reference is torch on the CPU in float64: conv2d -> activation -> pixel_shuffle -> + residual; autograd for
dx, a masked gradient masked by the tensor handed to the kernel.

Per row: the return code is 0 (a row the table says is refused: SRK_ERR_UNSUPPORTED, a message, the output still all NaN
between intact guards); srk_last_kernel_name() starts with the row's prefix (f16x3: ",f16" in it); no NaN left, guards
untouched; every element within the row's bar of float64 (assert_close_elementwise: atol = rtol * rms), pixel-shuffle rows
in the shuffled layout; the same call into a fresh buffer gives the same bits; srk_conv_result.bn_partial_rows == 0.
y_amax: the row says whether its kernel keeps the maximum (A: wrote_amax == 1, Z: wrote_amax == 0).  wrote_amax == 1 ->
the maximum over the slots equals max|y| of what was stored, exactly, and two
further calls: every slot pre-set to 2 max|y| stays as it is, every slot pre-set to 0.5 max|y| ends with the maximum max|y|;
with a residual, four more with 1000 added to the residual in one corner of the output each (the maximum sits in the first
or the last tile, whatever the tiling): the same equality;  wrote_amax == 0 -> every slot is still 0.
Bars, by the arithmetic that runs: 1e-4 for the bf16x3 class, TOL_TIGHT (2e-5) for bf16x6, f16x3, the exact-fp32 kernels and
k_conv_tapn with one tap group.

Measured on an MI355X (profiles/stride1_parity.txt has every row), worst error / bar: bf16x3 rows 0.05 .. 0.79 of 1e-4 (the
worst: k_conv_bf3's 4-wave blocks on the 131580-pixel rows), bf16x6 / f16x3 0.005 .. 0.09 of 2e-5, exact fp32 0.005 .. 0.16
of 2e-5.  The whole module: 356 cases in 5.4 s (tests/test_strided_gpu.py: 80 cases in 4 s)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stride1_epilogue_ref as R
from conftest import TOL_TIGHT, assert_close_elementwise
from conv_abi import Guarded, _nhwc, _pkg, _place, _ratio

pytestmark = pytest.mark.gpu

assert R.TOL_TIGHT == TOL_TIGHT
ALGOS = {"auto": 0, "generic": 1, "mfma_fp32": 2, "direct": 3, "bf16x3": 4, "bf16x6": 5, "f16x3": 6}
ACTS = {"none": None, "relu": "relu", "lrelu": "lrelu", "prelu1": "prelu", "preluC": "prelu", "tanh": "tanh", "sigmoid": "sigmoid"}


class _Problem(object):
    """The device tensors of one row and the call on them"""

    def __init__(self, c, gpu):
        pkg = _pkg()
        self.lib, self.L, self.ops = pkg._lib.load(), pkg._lib, pkg.ops
        lib, L = self.lib, self.L
        self.c, self.gpu = c, gpu
        r = self.r = R.ps_r(c)
        OH, OW = R.out_hw(c)
        assert OH == lib.srk_conv_out_dim(c.H, c.k, 1, c.p, 0, 0) and OW == lib.srk_conv_out_dim(c.W, c.k, 1, c.p, 0, 0)
        self.d = L.ConvDesc(c.N, c.H, c.W, c.cin, OH, OW, c.cout, c.k, c.k, 1, c.p, 0, 0, ALGOS[c.algo], int("N" in c.epi),
                            r if c.kind == "dgrad" else 0)
        t = R.tensors(c.id)
        wg = t["w"].to(gpu)
        self.b = self.pw = self.res = self.x_amax = self.ym = self.xr = None
        if c.kind == "fwd":
            self.wp = self.ops.pack_weight_fwd(wg, False, r)
            self.x = _place(t["x"].contiguous() if "N" in c.epi else _nhwc(t["x"]), gpu, R.off(c, "x"))
            if "b" in c.epi:
                self.b = _place(R.shuffle_bias(t["b"], r), gpu, R.off(c, "b"))
            if R.act(c) in ("prelu1", "preluC"):
                self.pw = t["pw"].to(gpu)
            if "r" in c.epi:
                self.res = _place(_nhwc(t["res"]), gpu, R.off(c, "r"))
            if c.algo == "f16x3":
                self.x_amax = torch.zeros(L.AMAX_FLOATS, dtype=torch.float32, device=gpu)
                L.check(lib.srk_absmax(L.ptr(self.x), self.x.numel(), L.ptr(self.x_amax), L.stream_ptr()), "srk_absmax")
            self.out_numel = c.N * OH * OW * c.cout
            self.out_shape = (c.N, OH * r, OW * r, c.cout // (r * r)) if r else (c.N, OH, OW, c.cout)
        else:
            self.wp = self.ops.pack_weight_bwd(wg, False, r)
            shuf = (lambda v: F.pixel_shuffle(v, r)) if r else (lambda v: v)
            self.x = _place(_nhwc(shuf(t["dy"])), gpu, R.off(c, "x"))
            if "m" in c.epi or "z" in c.epi:
                self.ym = _place(_nhwc(shuf(t["ym"])), gpu)
            if "a" in c.epi:
                self.res = _place(_nhwc(t["res"]), gpu, R.off(c, "r"))
            if "X" in c.epi:
                self.xr = _place(_nhwc(t["xr"]), gpu)
            self.out_numel, self.out_shape = c.N * c.H * c.W * c.cin, (c.N, c.H, c.W, c.cin)

    def call(self, out, y_amax=None):
        """the row's call into `out` -> (return code, srk_conv_result or None)"""
        lib, L, c = self.lib, self.L, self.c
        if c.kind == "fwd":
            a = R.act(c)
            ep = L.Epilogue(L.ptr(self.b), L.ptr(self.pw), L.ptr(self.res), R.SLOPE if a == "lrelu" else 0.0,
                            L.ACT_BY_NAME[ACTS[a]], 0 if self.pw is None else self.pw.numel(), self.r, L.ptr(self.x_amax),
                            L.ptr(y_amax), None)
            res = L.ConvResult()
            res.wrote_amax, res.bn_partial_rows = 7, 7
            rc = lib.srk_conv2d_forward_ex(ctypes.byref(self.d), L.ptr(self.x), L.ptr(self.wp), L.ptr(out.t), ctypes.byref(ep),
                                           ctypes.byref(res), L.stream_ptr())
            return rc, res
        m = L.BwdMask(L.ptr(self.ym), R.SLOPE if "m" in c.epi else 0.0)
        mref = ctypes.byref(m) if self.ym is not None else None
        if "X" in c.epi:
            return lib.srk_conv2d_backward_data_relu(ctypes.byref(self.d), L.ptr(self.x), L.ptr(self.wp), L.ptr(out.t), mref,
                                                     L.ptr(self.xr), L.stream_ptr()), None
        return lib.srk_conv2d_backward_data(ctypes.byref(self.d), L.ptr(self.x), L.ptr(self.wp), L.ptr(out.t), mref,
                                            L.ptr(self.res), L.stream_ptr()), None

    def run(self, what, y_amax=None):
        """the call into a fresh NaN-filled output -> (NCHW-ordered numpy result, kernel name, srk_conv_result)"""
        out = Guarded(self.out_numel, self.gpu, R.off(self.c, "y"))
        rc, res = self.call(out, y_amax)
        assert rc == 0, (what, rc, self.lib.srk_last_error_string().decode())
        name = self.lib.srk_last_kernel_name().decode()
        torch.cuda.synchronize()
        return out.check(what).reshape(self.out_shape).transpose(0, 3, 1, 2), name, res


@pytest.mark.parametrize("c", R.CASES, ids=[c.id for c in R.CASES])
def test_stride1_epilogue(gpu, monkeypatch, c):
    for k, v in c.env:
        monkeypatch.setenv(k, v)
    P = _Problem(c, gpu)
    L = P.L
    if c.prefix is None:      # a legal request that no kernel covers: refused before anything is launched
        out = Guarded(P.out_numel, gpu, R.off(c, "y"))
        rc, res = P.call(out)
        torch.cuda.synchronize()
        assert rc == L.ERR_UNSUPPORTED, (c.id, rc)
        assert P.lib.srk_last_error_string().decode() != "", c.id
        out.check_untouched(c.id)
        assert res is None or (res.wrote_amax, res.bn_partial_rows) == (0, 0)
        print("PARITY %-30s %-5s %-9s %-34s refused" % (c.id, c.kind, c.algo, "-"))
        return
    ref = R.reference(c.id)["out"].numpy()
    want_amax = "A" in c.epi or "Z" in c.epi
    ya = torch.zeros(L.AMAX_FLOATS, dtype=torch.float32, device=gpu) if want_amax else None
    got, name, res = P.run("A", ya)
    assert name.startswith(c.prefix), (c.id, name)
    if c.algo == "f16x3":
        assert ",f16" in name, name
    print("PARITY %-30s %-5s %-9s %-34s %.4f of %.0e" % (c.id, c.kind, c.algo, name, _ratio(got, ref, c.tol), c.tol))
    assert got.shape == ref.shape
    assert_close_elementwise(got, ref, c.tol, what=c.id)
    if res is not None:
        assert res.bn_partial_rows == 0, c.id
        assert want_amax or res.wrote_amax == 0, (c.id, res.wrote_amax)
    again, name2, _ = P.run("B")
    assert name2 == name
    assert np.array_equal(got, again), "%s: the second run differs" % c.id
    if not want_amax:
        return
    slots = ya.cpu().numpy().reshape(16, -1)[:, 0]
    rest = ya.cpu().numpy().reshape(16, -1)[:, 1:]
    assert (rest == 0).all(), "%s: floats between the slots were written" % c.id
    top = float(np.abs(got).max())
    assert res.wrote_amax == (1 if "A" in c.epi else 0), "%s: wrote_amax == %d" % (c.id, res.wrote_amax)
    if res.wrote_amax == 0:
        assert (slots == 0).all(), "%s: wrote_amax == 0, but the slots hold %s" % (c.id, slots[slots != 0])
        return
    assert float(slots.max()) == top, "%s: y_amax %.9g, max|y| %.9g" % (c.id, float(slots.max()), top)
    # slots that already hold a value: one above the maximum stays, one below is raised to it
    for factor in (2.0, 0.5):
        pre = np.float32(factor * top)
        yb = torch.full((L.AMAX_FLOATS,), float(pre), dtype=torch.float32, device=gpu)
        got2, _, res2 = P.run("amax x%g" % factor, yb)
        assert res2.wrote_amax == 1 and np.array_equal(got2, got)
        after = yb.cpu().numpy().reshape(16, -1)
        assert (after[:, 1:] == pre).all(), "%s: floats between the slots were written" % c.id
        if factor > 1:
            assert (after[:, 0] == pre).all(), "%s: a slot above max|y| was changed" % c.id
        else:
            assert float(after[:, 0].max()) == top and (after[:, 0] >= pre).all(), \
                "%s: slots pre-set to %.9g hold %s, max|y| %.9g" % (c.id, float(pre), after[:, 0], top)
    # a maximum planted in each corner of the output (rows with a residual): the first and the last tiles commit theirs too
    if P.res is None:
        return
    row = P.out_shape[2] * P.out_shape[3]
    for idx in (0, row - 1, P.out_numel - row, P.out_numel - 1):
        keep = float(P.res[idx])
        P.res[idx] = keep + 1000.0
        yc = torch.zeros(L.AMAX_FLOATS, dtype=torch.float32, device=gpu)
        got3, _, res3 = P.run("amax, planted at %d" % idx, yc)
        P.res[idx] = keep
        top3 = float(np.abs(got3).max())
        assert res3.wrote_amax == 1 and top3 > 500.0
        assert float(yc.max()) == top3, "%s: maximum planted at element %d: y_amax %.9g, max|y| %.9g" % (c.id, idx, float(yc.max()), top3)


def test_bf3_phases_that_differ_report_no_maximum(gpu, monkeypatch):
    """A strided transposed conv runs one k_conv_bf3 launch per output phase, and the phases of an odd-sized input differ by
    a row or a column: 363 x 363, k3 s2 p1 gives phases of 131769 / 131406 / 131406 / 131044 pixels either side of the 131072
    at which the launcher changes from the 2-wave blocks (no maximum) to <NT,4,vec> (keeps it).  A maximum over some of the
    phases would under-report max|y|: the call must say wrote_amax == 0 and leave the slots alone."""
    monkeypatch.setenv("SRK_BF3_DIRECT", "0")
    monkeypatch.setenv("SRK_BFW", "0")
    pkg = _pkg()
    lib, L, ops = pkg._lib.load(), pkg._lib, pkg.ops
    H = 363
    OH = lib.srk_conv_out_dim(H, 3, 2, 1, 1, 0)
    d = L.ConvDesc(1, H, H, 8, OH, OH, 32, 3, 3, 2, 1, 1, 0, ALGOS["auto"], 0, 0)
    x = torch.randn(H * H * 8, device=gpu)
    wp = ops.pack_weight_fwd(torch.randn(8, 32, 3, 3, device=gpu) * 0.1, True, 0)
    out = Guarded(OH * OH * 32, gpu)
    ya = torch.zeros(L.AMAX_FLOATS, dtype=torch.float32, device=gpu)
    ep = L.Epilogue(None, None, None, 0.0, L.ACT_BY_NAME[None], 0, 0, None, L.ptr(ya), None)
    res = L.ConvResult()
    rc = lib.srk_conv2d_forward_ex(ctypes.byref(d), L.ptr(x), L.ptr(wp), L.ptr(out.t), ctypes.byref(ep), ctypes.byref(res),
                                   L.stream_ptr())
    assert rc == 0, lib.srk_last_error_string().decode()
    assert lib.srk_last_kernel_name().decode().startswith("k_conv_bf3<"), lib.srk_last_kernel_name().decode()
    torch.cuda.synchronize()
    out.check("phases")
    assert res.wrote_amax == 0 and bool((ya == 0).all())
