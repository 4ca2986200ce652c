"""Every branch of the stride-1 bf16x3 weight gradient (csrc/conv_wgrad_bf16.hip: k_wgrad_bf in its three tile
configurations, per-tile and wave-specialised, both K loops, both staging modes, 16-byte and scalar loads, plain and
pixel-shuffled dY, single and grouped launches) against torch's float64 gradient, through the C ABI
(srk_conv2d_backward_weight[_grouped]) so that pointer alignment and db == NULL are the test's choice.  The shapes are
the table of tests/wgrad_plan_ref.py (CASES): the smallest batch at which the planner picks the row's variant on 256 CUs;
tests/test_wgrad_plan_cpu.py checks the table against the library's planner (srk_conv2d_backward_weight_plan), this module
checks table and planner against srk_last_kernel_name().  Then the exact-fp32 kernels (k_wgrad_mfma, algo = mfma_fp32) at the same shapes, where their
blocks walk more than one tile (ntiles ~ 500 .. 3000 against <= 512 slabs).

Inputs: oracle.fill.randn, the outermost two rows and columns of x, dY and the mask source times 4 (border and halo terms
dominate their taps); NHWC views cut from a flat allocation at a 16-byte boundary or the row's byte offset from one.

Per row, bf16x3:
  A  beta = 0 into NaN-filled dw / db between sentinel guards, the workspace exactly the size the library asks for and
     NaN-filled, 4 KB of sentinel bytes behind it: no NaN left, guards and tail untouched, the kernel name as in the table;
     dw element-wise within 1e-4 (TOL_ALGO["auto"], atol = rtol * rms) of float64, db within 2e-5 (max-norm)
  B  the same call again: bit-equal (split-K is deterministic by construction)
  C  beta = 1 onto a 0.5 / -0.25 fill: result minus fill within the same bars
  D  db = NULL (rows 1, 5, 10, 14 and the grouped rows): dw bit-equal to A
  grouped rows: each layer within 2e-5 of its own single-layer call
fp32 (rows without pixel-shuffled dY, single launches): A and B, dw element-wise within TOL_TIGHT (2e-5), db within 2e-5.

Which row runs which kernel / branch (k_wgrad_bf<CIT,COW,NTW,...>; "plain" = stage() called from the spec loop)
  <4,1,2,spec>  K33, plain (64-channel X chunk > register batch)      1 espcn2 (TH 12, 3 tile columns, ragged right, ReLU mask),
                                                                      2 cout_tail (24 of 32 columns, TWo 3), 3 two_cin_chunks
                                                                      (64 + 16 channels, swizzled grid, LeakyReLU), 22 ps2_C8
                generic loop 2x2, plain                               24 k2x2
                K33, prefetch + ring, one tile row, 84 idle blocks    4 one_tile_row
                generic loop 1x1, prefetch + ring (HH == TH)          9 srcnn_1x1 (TWo 5, TH 3)
                scalar dY + mask loads (4 bytes off)                  19 dy_unaligned
                grouped                                               28 grp_64_32 (middle layer unmasked)
  <4,1,1,spec>  K33, plain                                            5 fsrcnn_map, 6 fsrcnn_map_nopad (exact tiles), 23 ps2_C4
                generic loop 2x2 pad 1 / 3x1 pad 1, plain             25 k2x2_pad (TH 14), 27 k3x1 (OW = W + 2)
                generic loop 1x1, prefetch + ring                     7 fsrcnn_shrink, 30 grp_1x1
                scalar loads with a 2-channel tail: x and dY / x / dY 14 c10_10, 15 c10_12, 16 c12_10, 32 grp_scalar
                grouped                                               29 grp_12_12
  <2,2,2,spec>  K33, prefetch + ring, not k_wgrad_tr                  10 espcn3 (48 of 64 columns), 11 c48_64 (32 + 16 channels,
                                                                      swizzle, idle blocks), 12 c80_64 (three chunks, G 85),
                                                                      13 c32_80 (two column blocks), 21 ps2_C16, 31 grp_48_64
                generic loop 1x1 / 1x3, prefetch + ring               8 fsrcnn_expand, 26 k1x3 (two chunks)
                scalar: 1-channel tails / x / mask off a boundary     17 c9_33, 18 x_unaligned, 20 mask_unaligned
  <.,tile>      swizzled grid / scalar tail / unaligned / ps dY       33 tile_swizzle, 34 tile_scalar, 35 tile_unaligned,
                                                                      36 tile_ps_C16
(`prefetch` without `ring` cannot be planned: the static_assert of csrc/conv_wgrad_plan.h, and
test_wgrad_plan_cpu.py::test_no_plannable_tile_prefetches_without_the_ring.)

Measured on an MI355X (profiles/wgrad_bf_parity.txt has every row), worst error / bar:
  bf16x3  dw  0.087 (row 25) .. 0.211 (row 34) of the 1e-4 bar (a CPU emulation of the 3-term split: 0.12 .. 0.14)
          db  0.003 (row 16) .. 0.018 (row 32) of 2e-5
  fp32    dw  0.022 (row 34) .. 0.043 (row 5) of 2e-5;  db 0.004 .. 0.013 of 2e-5
The whole module: 63 cases in 7 s."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_plan_ref as R
from conftest import TOL_TIGHT, assert_close_elementwise, rel_err
from oracle import fill

pytestmark = pytest.mark.gpu

TOL_BF = 1e-4          # test_ops_gpu.TOL_ALGO["auto"]
TOL_DB = 2e-5
GUARD = 64
SENT = -12345.5
TAIL = 4096
DB_NULL_ROWS = (1, 5, 10, 14)
SLOPE = {None: 0.0, "relu": 0.0, "lrelu": 0.2}


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _edges_x4(t):
    """NCHW tensor with its outermost two rows and columns multiplied by 4"""
    H, W = t.shape[2], t.shape[3]
    m = torch.ones(H, W)
    m[:2], m[-2:], m[:, :2], m[:, -2:] = 4.0, 4.0, 4.0, 4.0
    return t * m


@functools.lru_cache(maxsize=8)
def _inputs(cid, layer):
    """-> x [N, Cin, H, W], dy [N, Cout, OH, OW], mask source y (or None): float32, NCHW index order"""
    c = R.BY_ID[cid]
    OH, OW = R.out_dims(c.H, c.W, c.kh, c.kw, c.pad)
    seed = 7000 + 100 * c.row + 10 * layer
    x = _edges_x4(fill.randn((c.N, c.cin, c.H, c.W), seed))
    dy = _edges_x4(fill.randn((c.N, c.cout, OH, OW), seed + 1))
    y = _edges_x4(fill.randn((c.N, c.cout, OH, OW), seed + 2)) if R.layer_mask(c, layer) else None
    return x, dy, y


@functools.lru_cache(maxsize=None)
def _reference(cid, layer):
    """torch's float64 weight / bias gradient of the layer, the masked dY formed in float64 -> numpy (dw, db)"""
    c = R.BY_ID[cid]
    x, dy, y = _inputs(cid, layer)
    dym = dy.double()
    if y is not None:
        dym = torch.where(y > 0, dym, dym * SLOPE[R.layer_mask(c, layer)])
    wr = torch.zeros(c.cout, c.cin, c.kh, c.kw, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(c.cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wr, br, 1, c.pad).backward(dym)
    return wr.grad.numpy().copy(), br.grad.numpy().copy()


def _place(t, gpu, off=0):
    """a flat device copy of t, `off` bytes past a 16-byte boundary inside one allocation"""
    assert off % 4 == 0 and 0 <= off < 16
    flat = t.reshape(-1)
    big = torch.empty(flat.numel() + 4, dtype=torch.float32, device=gpu)
    assert big.data_ptr() % 16 == 0
    v = big[off // 4: off // 4 + flat.numel()]
    v.copy_(flat)
    assert v.data_ptr() % 16 == off and v.numel() == flat.numel()
    return v


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


class Guarded(object):
    """n floats at a 16-byte boundary inside one allocation, GUARD sentinel floats either side (the pattern of
    tests/test_streaming_gpu.py); NaN-filled, or filled with `init`"""

    def __init__(self, n, gpu, init=None):
        self.n = n
        self.big = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float32, device=gpu)
        self.t = self.big[GUARD:GUARD + n]
        assert self.t.data_ptr() % 16 == 0
        self.t.fill_(float("nan") if init is None else init)

    def check(self, what):
        big = self.big.cpu().numpy()
        lo, hi = GUARD, GUARD + self.n
        assert (big[:lo] == np.float32(SENT)).all() and (big[hi:] == np.float32(SENT)).all(), "%s: a guard was written" % what
        assert not np.isnan(big[lo:hi]).any(), "%s: %d elements never written" % (what, int(np.isnan(big[lo:hi]).sum()))
        return big[lo:hi].copy()


class _Problem(object):
    """The device tensors of one row and the calls on them"""

    def __init__(self, c, gpu, algo=0):
        pkg = _pkg()
        self.lib, self.L = pkg._lib.load(), pkg._lib
        self.c, self.gpu = c, gpu
        OH, OW = R.out_dims(c.H, c.W, c.kh, c.kw, c.pad)
        assert OH == self.lib.srk_conv_out_dim(c.H, c.kh, 1, c.pad, 0, 0) and OW == self.lib.srk_conv_out_dim(c.W, c.kw, 1, c.pad, 0, 0)
        self.d = self.L.ConvDesc(c.N, c.H, c.W, c.cin, OH, OW, c.cout, c.kh, c.kw, 1, c.pad, 0, 0, algo, 0, c.ps)
        self.xs, self.dys, self.ys, self.slopes = [], [], [], []
        for l in range(c.n):
            x, dy, y = _inputs(c.id, l)
            if c.ps > 1:   # the gradient as the pixel-shuffle's input gradient would arrive: [N, C / r^2, OH r, OW r]
                dy = F.pixel_shuffle(dy, c.ps)
            self.xs.append(_place(_nhwc(x), gpu, c.off[0]))
            self.dys.append(_place(_nhwc(dy), gpu, c.off[1]))
            self.ys.append(None if y is None else _place(_nhwc(y), gpu, c.off[2]))
            self.slopes.append(SLOPE[R.layer_mask(c, l)])
        self.numel = c.cout * c.cin * c.kh * c.kw

    def _ws(self, nbytes):
        assert nbytes > 0
        ws = torch.full((nbytes + TAIL,), 0xFF, dtype=torch.uint8, device=self.gpu)     # as floats: NaN everywhere
        assert ws.data_ptr() % 16 == 0
        return ws

    def _mask(self, l):
        return self.L.BwdMask(None if self.ys[l] is None else self.ys[l].data_ptr(), self.slopes[l])

    def single(self, l, beta, want_db, what):
        """srk_conv2d_backward_weight of layer l -> dw [Cout, Cin, KH, KW], db (or None), kernel name"""
        lib, L, c = self.lib, self.L, self.c
        init = None if beta == 0.0 else (0.5, -0.25)
        dw = Guarded(self.numel, self.gpu, init and init[0])
        db = Guarded(c.cout, self.gpu, init and init[1]) if want_db else None
        nbytes = int(lib.srk_conv2d_backward_weight_workspace_bytes(ctypes.byref(self.d)))
        ws = self._ws(nbytes)
        m = self._mask(l)
        L.check(lib.srk_conv2d_backward_weight(ctypes.byref(self.d), L.ptr(self.xs[l]), L.ptr(self.dys[l]),
                                               ctypes.byref(m) if self.ys[l] is not None else None, L.ptr(dw.t),
                                               L.ptr(db.t) if db else None, beta, L.ptr(ws), nbytes, L.stream_ptr()), what)
        name = lib.srk_last_kernel_name().decode()
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xFF).all()), "%s: bytes behind the workspace were written" % what
        return (dw.check(what + " dw").reshape(c.cout, c.cin, c.kh, c.kw), db.check(what + " db") if db else None, name)

    def grouped(self, beta, want_db, what):
        """srk_conv2d_backward_weight_grouped over all layers -> [dw], [db] (or None), kernel name"""
        lib, L, c, n = self.lib, self.L, self.c, self.c.n
        init = None if beta == 0.0 else (0.5, -0.25)
        dws = [Guarded(self.numel, self.gpu, init and init[0]) for _ in range(n)]
        dbs = [Guarded(c.cout, self.gpu, init and init[1]) for _ in range(n)] if want_db else None
        vp = ctypes.c_void_p
        arr = lambda ts: (vp * n)(*[None if t is None else t.data_ptr() for t in ts])
        masks = (L.BwdMask * n)(*[self._mask(l) for l in range(n)])
        nbytes = int(lib.srk_conv2d_backward_weight_grouped_workspace_bytes(ctypes.byref(self.d), n))
        ws = self._ws(nbytes)
        L.check(lib.srk_conv2d_backward_weight_grouped(ctypes.byref(self.d), n, arr(self.xs), arr(self.dys), masks,
                                                       arr([g.t for g in dws]), arr([g.t for g in dbs]) if dbs else None,
                                                       beta, L.ptr(ws), nbytes, L.stream_ptr()), what)
        name = lib.srk_last_kernel_name().decode()
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xFF).all()), "%s: bytes behind the workspace were written" % what
        shape = (c.cout, c.cin, c.kh, c.kw)
        return ([g.check("%s dw[%d]" % (what, l)).reshape(shape) for l, g in enumerate(dws)],
                [g.check("%s db[%d]" % (what, l)) for l, g in enumerate(dbs)] if dbs else None, name)

    def run(self, beta, want_db, what):
        """the row's own entry point -> [dw], [db] or None, name"""
        if self.c.n > 1:
            return self.grouped(beta, want_db, what)
        dw, db, name = self.single(0, beta, want_db, what)
        return [dw], None if db is None else [db], name


def _ratio(got, ref, rtol):
    """worst |got - ref| / (atol + rtol |ref|), atol = rtol * rms(ref): how much of assert_close_elementwise's bar is used"""
    ref = np.asarray(ref, np.float64)
    atol = rtol * float(np.sqrt(np.mean(ref * ref)))
    return float((np.abs(np.asarray(got, np.float64) - ref) / (atol + rtol * np.abs(ref))).max())


def _check_against_fp64(c, dws, dbs, rtol, arith, what, shift=(0.0, 0.0)):
    for l in range(c.n):
        rw, rb = _reference(c.id, l)
        dw = dws[l].astype(np.float64) - shift[0]
        assert np.isfinite(dw).all()
        line = "PARITY row %2d %-16s %-6s %-6s layer %d  dw %.4f of %.0e" % (c.row, c.id, arith, what, l, _ratio(dw, rw, rtol), rtol)
        if dbs is not None:
            db = dbs[l].astype(np.float64) - shift[1]
            assert np.isfinite(db).all()
            line += "  db %.4f of %.0e" % (rel_err(db, rb) / TOL_DB, TOL_DB)
        print(line)
        assert_close_elementwise(dw, rw, rtol, what="%s %s dw[%d]" % (c.id, what, l))
        if dbs is not None:
            assert rel_err(db, rb) < TOL_DB, (c.id, what, l)


@pytest.mark.parametrize("c", R.CASES, ids=["%02d_%s" % (c.row, c.id) for c in R.CASES])
def test_wgrad_bf_plan_branches(gpu, c):
    P = _Problem(c, gpu)
    # A: beta = 0 into NaN, exact workspace; the kernel the row is in the table for
    dwA, dbA, name = P.run(0.0, True, "A")
    assert name == c.name, (c.row, name)
    assert name == R.plan_case(c).name
    _check_against_fp64(c, dwA, dbA, TOL_BF, "bf16x3", "A")
    # B: again -> the same bits
    dwB, dbB, _ = P.run(0.0, True, "B")
    for l in range(c.n):
        assert np.array_equal(dwA[l], dwB[l]) and np.array_equal(dbA[l], dbB[l]), l
    # C: beta = 1 accumulates onto what the tensors held
    dwC, dbC, _ = P.run(1.0, True, "C")
    _check_against_fp64(c, dwC, dbC, TOL_BF, "bf16x3", "C", shift=(0.5, -0.25))
    # D: without a bias gradient the weight gradient is the same
    if c.n > 1 or c.row in DB_NULL_ROWS:
        dwD, dbD, nameD = P.run(0.0, False, "D")
        assert dbD is None and nameD == name
        for l in range(c.n):
            assert np.array_equal(dwA[l], dwD[l]), l
    # grouped: every layer against its own single-layer call (same kernels, other split-K counts)
    if c.n > 1:
        for l in range(c.n):
            dw1, db1, name1 = P.single(l, 0.0, True, "single[%d]" % l)
            assert name1.startswith("k_wgrad_bf<") and "grouped" not in name1, name1
            assert rel_err(dwA[l], dw1) < 2e-5 and rel_err(dbA[l], db1) < 2e-5, l


FP32_CASES = [c for c in R.CASES if c.ps == 0 and c.n == 1]


@pytest.mark.parametrize("c", FP32_CASES, ids=["%02d_%s" % (c.row, c.id) for c in FP32_CASES])
def test_wgrad_fp32_same_shapes(gpu, c):
    """k_wgrad_mfma (algo = mfma_fp32) at the rows' shapes: its blocks walk several tiles here, which no KAT size does"""
    P = _Problem(c, gpu, algo=2)
    dwA, dbA, name = P.run(0.0, True, "A")
    assert name.startswith("k_wgrad_mfma<%d,conv>" % min(4, (c.cout + 15) // 16)), (c.row, name)
    _check_against_fp64(c, dwA, dbA, TOL_TIGHT, "fp32", "A")
    dwB, dbB, _ = P.run(0.0, True, "B")
    assert np.array_equal(dwA[0], dwB[0]) and np.array_equal(dbA[0], dbB[0])
