"""Strided and transposed convolutions, every phase geometry, against float64 (through the C ABI: srk_conv2d_forward,
srk_conv2d_backward_data, srk_conv2d_backward_weight).

A ConvTranspose2d forward and the data gradient of a strided Conv2d are TRANS gathers that csrc/conv_tile.h for_each_phase
splits into s x s output phases, each with its own tap count, output origin, extent, input origin and reversed weight
walk; every conv family consumes those parameters.  The rows are the table of tests/strided_phase_ref.py (CASES; its
docstring names the edges, tests/test_strided_phase_cpu.py checks each row's against the library's own phase decomposition):
zero-tap phases, skipped phases, phases of several ragged tiles, unequal tap counts, dx rows no dy reaches, the phased
store under bias / LeakyReLU / per-channel PReLU / residual, unaligned tensors -- on k_conv_bfd_mp, k_conv_bfd (small
block with 1 .. 4 channel waves, the large blocks, bf16x3 / bf16x6 / f16x3), k_conv_bf3, k_conv_tapn (one tap group and
several), k_conv_direct, k_conv_mfma, k_conv_mfma_tg, k_gather_conv, and k_wgrad_mfma<.,trans|conv> / k_wgrad_mfma_smallcin / k_wgrad_generic.

Inputs: oracle.fill.randn, the outermost two rows and columns of x and dy times 4; NHWC tensors cut from one flat
allocation at a 16-byte boundary (or the row's byte offset past one); outputs NaN-filled between sentinel guards; the
weight-gradient workspace exactly the size the library asks for, NaN-filled, 4 KB of sentinel behind it.  The reference is
torch's conv_transpose2d / conv2d in float64 on the CPU, autograd for the gradients; a masked gradient is masked by the
tensor handed to the kernel (dy * (y > 0 ? 1 : slope) formed in float64), not by a forward of the reference.

Per call: return code 0, no NaN left, guards (and the workspace tail) untouched, srk_last_kernel_name() starts with the
row's prefix, every element within the row's bar of float64 (assert_close_elementwise: atol = rtol * rms), and the same
call again into a fresh NaN-filled buffer gives the same bits (k_wgrad_generic sums with float atomics: no such clause,
max-norm bar); dw and db of the other weight-gradient rows are both held element-wise.  Bars, by the arithmetic that runs: 1e-4 for the bf16x3 class (TOL_ALGO["auto"]), TOL_TIGHT (2e-5) for
bf16x6, f16x3 and the exact-fp32 kernels.  k_conv_tapn runs the exact 3-way split in every class while the taps fit one
32-column group (TOL_TIGHT, as test_conv_few_output_channels holds it); with several tap groups it runs bf16x3 under
SRK_ALGO_AUTO (1e-4) and the exact split under SRK_ALGO_MFMA_BF16X6 (TOL_TIGHT).
Exact values: the outputs of a zero-tap phase are act(bias) + residual computed in fp32, bit for bit; dx elements that
no dy reaches (k1 s2: the odd positions; k3 s2 p0: the trailing row / column) are exactly 0.0, or exactly add_to.

Measured on an MI355X (profiles/strided_parity.txt has every row), worst error / bar: bf16x3 rows 0.12 .. 0.47 of 1e-4,
bf16x6 / f16x3 0.01 .. 0.06 of 2e-5, exact fp32 0.01 .. 0.07 of 2e-5, k_wgrad_mfma dw below 0.025 and db below 0.012 of 2e-5.
The whole module: 80 cases in 4 s."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import strided_phase_ref as R
from conftest import TOL_TIGHT, assert_close_elementwise, rel_err
from conv_abi import Guarded, _edges_x4, _nhwc, _pkg, _place, _ratio
from oracle import fill

pytestmark = pytest.mark.gpu

assert R.TOL_TIGHT == TOL_TIGHT
ALGOS = {"auto": 0, "generic": 1, "mfma_fp32": 2, "bf16x6": 5, "f16x3": 6}
TAIL = 4096
SLOPE = 0.2


@functools.lru_cache(maxsize=4)
def _tensors(cid):
    """float32, NCHW index order: x, w (torch layout), bias, PReLU slopes, residual / add_to (of the call's output), dy,
    the mask source y (dy's shape)"""
    c = R.BY_ID[cid]
    OH, OW = R.dims(c)
    seed = 9000 + 20 * [k.id for k in R.CASES].index(cid)
    x = _edges_x4(fill.randn((c.N, c.cin, c.H, c.W), seed))
    wshape = (c.cin, c.cout, c.kh, c.kw) if c.tr else (c.cout, c.cin, c.kh, c.kw)
    # (fan-in of a transposed conv's output element: about Cin * taps / s^2)
    fan = c.cin * max(1, c.kh * c.kw // (c.s * c.s if c.tr else 1))
    w = fill.randn(wshape, seed + 1, (2.0 / fan) ** 0.5)
    b = fill.randn((c.cout,), seed + 2, 0.1)
    pw = 0.25 + 0.05 * fill.randn((c.cout,), seed + 3)
    out_shape = (c.N, c.cout, OH, OW) if c.kind == "fwd" else (c.N, c.cin, c.H, c.W)
    res = fill.randn(out_shape, seed + 4)
    dy = _edges_x4(fill.randn((c.N, c.cout, OH, OW), seed + 5))
    y = _edges_x4(fill.randn((c.N, c.cout, OH, OW), seed + 6))
    return x, w, b, pw, res, dy, y


def _conv64(c, x, w, b):
    if c.tr:
        return F.conv_transpose2d(x, w, b, c.s, c.p, c.op)
    return F.conv2d(x, w, b, c.s, c.p)


@functools.lru_cache(maxsize=None)
def _reference(cid):
    """float64, NCHW: fwd -> y;  dgrad -> dx;  wgrad -> (dw, db)"""
    c = R.BY_ID[cid]
    x, w, b, pw, res, dy, y = _tensors(cid)
    if c.kind == "fwd":
        r = _conv64(c, x.double(), w.double(), b.double() if "b" in c.epi else None)
        if "l" in c.epi:
            r = F.leaky_relu(r, SLOPE)
        if "P" in c.epi:
            r = F.prelu(r, pw.double())
        if "r" in c.epi:
            r = r + res.double()
        return r.numpy().copy()
    dym = dy.double()
    if "m" in c.epi:
        dym = torch.where(y > 0, dym, dym * SLOPE)
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    br = b.double().requires_grad_(True)
    _conv64(c, xr, wr, br).backward(dym)
    if c.kind == "dgrad":
        dx = xr.grad
        if "a" in c.epi:
            dx = dx + res.double()
        return dx.numpy().copy()
    return wr.grad.numpy().copy(), br.grad.numpy().copy()


class _Problem(object):
    """The device tensors of one row and the calls on them"""

    def __init__(self, c, gpu):
        pkg = _pkg()
        self.lib, self.L, self.ops = pkg._lib.load(), pkg._lib, pkg.ops
        lib = self.lib
        self.c, self.gpu = c, gpu
        OH, OW = R.dims(c)
        assert OH == lib.srk_conv_out_dim(c.H, c.kh, c.s, c.p, c.tr, c.op) and OW == lib.srk_conv_out_dim(c.W, c.kw, c.s, c.p, c.tr, c.op)
        self.OH, self.OW = OH, OW
        self.d = self.L.ConvDesc(c.N, c.H, c.W, c.cin, OH, OW, c.cout, c.kh, c.kw, c.s, c.p, c.tr, c.op, ALGOS[c.algo], 0, 0)
        x, w, b, pw, res, dy, y = _tensors(c.id)
        wg = w.to(gpu)
        if c.kind == "fwd":
            self.wp = self.ops.pack_weight_fwd(wg, bool(c.tr), 0)
            self.x = _place(_nhwc(x), gpu, c.off[0])
            self.b = b.to(gpu) if "b" in c.epi else None
            self.pw = pw.to(gpu) if "P" in c.epi else None
            self.res = _place(_nhwc(res), gpu) if "r" in c.epi else None
            self.amax = None
            if c.algo == "f16x3":
                self.amax = torch.zeros(self.L.AMAX_FLOATS, dtype=torch.float32, device=gpu)
                self.L.check(lib.srk_absmax(self.L.ptr(self.x), self.x.numel(), self.L.ptr(self.amax), self.L.stream_ptr()), "srk_absmax")
            self.out_numel, self.out_shape = c.N * OH * OW * c.cout, (c.N, OH, OW, c.cout)
        elif c.kind == "dgrad":
            self.wp = self.ops.pack_weight_bwd(wg, bool(c.tr), 0)
            self.dy = _place(_nhwc(dy), gpu, c.off[0])
            self.y = _place(_nhwc(y), gpu) if "m" in c.epi else None
            self.res = _place(_nhwc(res), gpu) if "a" in c.epi else None
            self.out_numel, self.out_shape = c.N * c.H * c.W * c.cin, (c.N, c.H, c.W, c.cin)
        else:
            self.x = _place(_nhwc(x), gpu)
            self.dy = _place(_nhwc(dy), gpu)
            self.y = _place(_nhwc(y), gpu) if "m" in c.epi else None
            self.w_shape = tuple(w.shape)

    def gather(self, what):
        """the row's forward or data-gradient call into a fresh NaN-filled output -> (NCHW-ordered numpy result, kernel name)"""
        lib, L, c = self.lib, self.L, self.c
        out = Guarded(self.out_numel, self.gpu, c.off[1])
        if c.kind == "fwd":
            act = L.ACT_LRELU if "l" in c.epi else (L.ACT_PRELU if "P" in c.epi else L.ACT_NONE)
            ep = L.Epilogue(L.ptr(self.b), L.ptr(self.pw), L.ptr(self.res), SLOPE if "l" in c.epi else 0.0, act,
                            c.cout if "P" in c.epi else 0, 0, L.ptr(self.amax), None, None)
            rc = lib.srk_conv2d_forward(ctypes.byref(self.d), L.ptr(self.x), L.ptr(self.wp), L.ptr(out.t), ctypes.byref(ep),
                                        L.stream_ptr())
        else:
            m = L.BwdMask(L.ptr(self.y), SLOPE)
            rc = lib.srk_conv2d_backward_data(ctypes.byref(self.d), L.ptr(self.dy), L.ptr(self.wp), L.ptr(out.t),
                                              ctypes.byref(m) if self.y is not None else None, L.ptr(self.res), L.stream_ptr())
        assert rc == 0, (what, rc, lib.srk_last_error_string().decode())
        name = lib.srk_last_kernel_name().decode()
        torch.cuda.synchronize()
        return out.check(what).reshape(self.out_shape).transpose(0, 3, 1, 2), name

    def wgrad(self, beta, want_db, what):
        """srk_conv2d_backward_weight -> dw (torch layout), db or None, kernel name"""
        lib, L, c = self.lib, self.L, self.c
        init = None if beta == 0.0 else (0.5, -0.25)
        dw = Guarded(int(np.prod(self.w_shape)), self.gpu, 0, init and init[0])
        db = Guarded(c.cout, self.gpu, 0, init and init[1]) if want_db else None
        nbytes = int(lib.srk_conv2d_backward_weight_workspace_bytes(ctypes.byref(self.d)))
        assert nbytes > 0
        ws = torch.full((nbytes + TAIL,), 0xFF, dtype=torch.uint8, device=self.gpu)     # as floats: NaN everywhere
        assert ws.data_ptr() % 16 == 0
        m = L.BwdMask(L.ptr(self.y), SLOPE)
        rc = lib.srk_conv2d_backward_weight(ctypes.byref(self.d), L.ptr(self.x), L.ptr(self.dy),
                                            ctypes.byref(m) if self.y is not None else None, L.ptr(dw.t),
                                            L.ptr(db.t) if db else None, beta, L.ptr(ws), nbytes, L.stream_ptr())
        assert rc == 0, (what, rc, lib.srk_last_error_string().decode())
        name = lib.srk_last_kernel_name().decode()
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xFF).all()), "%s: bytes behind the workspace were written" % what
        return dw.check(what + " dw").reshape(self.w_shape), db.check(what + " db") if db else None, name


def _exact_expected(c):
    """fp32 values the kernel must produce, bit for bit, where no input reaches the output (NCHW order) -> (mask [OH, OW],
    expected [N, C, OH, OW])"""
    x, w, b, pw, res, dy, y = _tensors(c.id)
    mask = np.array(R.untouched(c), dtype=bool)
    if c.kind == "fwd":
        OH, OW = R.dims(c)
        v = np.zeros((c.N, c.cout, OH, OW), dtype=np.float32)
        if "b" in c.epi:
            v = v + b.numpy()[None, :, None, None]
        if "l" in c.epi:
            v = np.where(v > 0, v, (np.float32(SLOPE) * v).astype(np.float32))
        if "r" in c.epi:
            v = (v + res.numpy()).astype(np.float32)
        return mask, v.astype(np.float32)
    v = res.numpy() if "a" in c.epi else np.zeros((c.N, c.cin, c.H, c.W), dtype=np.float32)
    return mask, v


GATHER_CASES = [c for c in R.CASES if c.kind != "wgrad"]
WGRAD_CASES = [c for c in R.CASES if c.kind == "wgrad"]


@pytest.mark.parametrize("c", GATHER_CASES, ids=[c.id for c in GATHER_CASES])
def test_strided_gather(gpu, monkeypatch, c):
    for k, v in c.env:
        monkeypatch.setenv(k, v)
    P = _Problem(c, gpu)
    ref = _reference(c.id)
    got, name = P.gather("A")
    assert name.startswith(c.prefix), (c.id, name)
    if c.algo == "f16x3":
        assert ",f16" in name, name
    if c.prefix.startswith("k_conv_bfd_mp<"):
        assert name.endswith("x%d" % len(R.case_phases(c))), name
    print("PARITY %-24s %-5s %-9s %-32s %.4f of %.0e" % (c.id, c.kind, c.algo, name, _ratio(got, ref, c.tol), c.tol))
    assert_close_elementwise(got, ref, c.tol, what=c.id)
    if c.exact:
        mask, want = _exact_expected(c)
        assert mask.any() and not mask.all()
        bad = (got != want)[:, :, mask]
        assert not bad.any(), "%s: %d of %d untouched elements are not the epilogue of zero" % (c.id, int(bad.sum()), bad.size)
    again, name2 = P.gather("B")
    assert name2 == name
    assert np.array_equal(got, again), "%s: the second run differs" % c.id


@pytest.mark.parametrize("c", WGRAD_CASES, ids=[c.id for c in WGRAD_CASES])
def test_strided_weight_gradient(gpu, c):
    P = _Problem(c, gpu)
    rw, rb = _reference(c.id)
    atomic = c.id in R.ATOMIC_ROWS

    def check(dw, db, name, what, shift=(0.0, 0.0)):
        dw = dw.astype(np.float64) - shift[0]
        db = db.astype(np.float64) - shift[1]
        if atomic:
            print("PARITY %-24s wgrad %-9s %-32s dw %.4f db %.4f of %.0e (max-norm) %s"
                  % (c.id, c.algo, name, rel_err(dw, rw) / c.tol, rel_err(db, rb) / c.tol, c.tol, what))
            assert rel_err(dw, rw) < c.tol and rel_err(db, rb) < c.tol
        else:
            print("PARITY %-24s wgrad %-9s %-32s dw %.4f of %.0e db %.4f of %.0e %s"
                  % (c.id, c.algo, name, _ratio(dw, rw, c.tol), c.tol, _ratio(db, rb, c.tol), c.tol, what))
            assert_close_elementwise(dw, rw, c.tol, what="%s %s dw" % (c.id, what))
            assert_close_elementwise(db, rb, c.tol, what="%s %s db" % (c.id, what))

    dwA, dbA, name = P.wgrad(0.0, True, "A")
    assert name.startswith(c.prefix), (c.id, name)
    check(dwA, dbA, name, "beta=0")
    if not atomic:
        dwB, dbB, _ = P.wgrad(0.0, True, "B")
        assert np.array_equal(dwA, dwB) and np.array_equal(dbA, dbB), "%s: the second run differs" % c.id
    dwC, dbC, nameC = P.wgrad(1.0, True, "C")
    assert nameC == name
    check(dwC, dbC, name, "beta=1", shift=(0.5, -0.25))
    if "n" in c.epi:
        dwD, dbD, nameD = P.wgrad(0.0, False, "D")
        assert dbD is None and nameD == name
        assert np.array_equal(dwA, dwD), "%s: dw differs without a bias gradient" % c.id
