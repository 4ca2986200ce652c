"""Every form of the streaming entry points (csrc/elementwise.hip, loss_optim.hip, prepost.hip, drcn.hip and the one-block
finals of ssim.hip / ssim_loss.hip) gives the parent commit's results, bit for bit: the kernels share one body per
operator (Vec<V>), one grid rule and one partial-sum finish, which may change where an operation is written
but never which operations run, in which order, or on how many blocks.  The goldens under tests/golden/streaming_bits/
were written by tools/streaming_golden.py with the parent commit's library; tensors up to 64 KB are kept whole, larger
ones as the SHA-256 of their bytes and their last 1024 elements.  Everything is compared as uint32.

Each form runs at two sizes: two to three blocks with a ragged last pass (NV floats for a 16-byte form, NS = NV + 3 for a
4-byte one, and NV floats one float off a 16-byte boundary: the 4-byte form at n % 4 == 0), and the first size above the
form's grid cap (streaming_ref.CAP_*), where the grid-stride loop wraps and the partial count saturates.  k_sgd<4>'s
65535-block cap is not swept (> 500 MB per buffer).

Not compared: what depends on the order of float atomics.  The single-slope PReLU gradient is compared only where at most
two blocks add into a zeroed slot (a + b == b + a; see test_train_gpu.test_srgan_step_is_its_segments_run_in_order); the
per-channel one is left to test_streaming_gpu's fp64 bar.  k_absmax's atomicMax does not depend on the order."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import streaming_ref as R
from streaming_ref import f32
from pytorch_super_resolution_model_collection_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streaming_bits")
WHOLE_BYTES = 64 * 1024
CORNER = 1024
NV, NS = 2448, 2451     # > 2048 (the largest per-block count of these kernels), NV % 4 == 0, NS % 4 == 3
TILE = 1 << 20          # a generator's output is repeated above this size (the values matter, not their number)
P, S = _lib.ptr, _lib.stream_ptr

CASES = {}
_KEEP = []              # every device buffer of the running case: none is handed back to the allocator (and to the next
                        # buffer of the case) while a launch that reads it is still to come


def case(name):
    def deco(fn):
        assert name not in CASES
        CASES[name] = fn
        return fn
    return deco


def _gen(fn, n, *a, **k):
    """fn(n, ...) of streaming_ref, every array cut or repeated to n elements"""
    out = fn(min(n, TILE), *a, **k)

    def fit(x):
        return [fit(y) for y in x] if isinstance(x, (list, tuple)) else np.resize(x, n)
    return fit(out)


def _dev(a, off=0):
    """the float32 values `a` on the device, `off` floats past a 16-byte boundary"""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    base = torch.zeros(a.size + 4, device="cuda")
    _KEEP.append(base)
    v = base[off:off + a.size]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * off and v.numel() == a.size
    return v


def _out(n, off=0, fill=float("nan")):
    base = torch.full((n + 4,), fill, device="cuda")
    _KEEP.append(base)
    v = base[off:off + n]
    assert v.data_ptr() % 16 == 4 * off and v.numel() == n
    return v


def _ws(nbytes):
    _KEEP.append(torch.empty(int(nbytes), dtype=torch.uint8, device="cuda"))
    return _KEEP[-1]


def _ok(rc):
    assert rc == 0, _lib.load().srk_last_error_string()


def _forms(cap4, cap1):
    """(tag, n, off) of one operator: both forms at the small sizes and just above their caps (None: no such size)"""
    out = [("v4", NV, 0), ("v1", NS, 0), ("v1off", NV, 1)]
    if cap4:
        out.append(("v4cap", cap4 + 4, 0))
    if cap1:
        out.append(("v1cap", cap1 + 3, 0))
    return out


# ---- SGD -----------------------------------------------------------------------------------------------------------------
SGD = {"plain": dict(mom=0.0, wd=0.0, nesterov=0, first=0, lr_dev=False, gs=None),
       "momentum_first": dict(mom=f32(0.9), wd=0.0, nesterov=0, first=1, lr_dev=True, gs=0.25),
       "momentum_later": dict(mom=f32(0.9), wd=0.0, nesterov=0, first=0, lr_dev=False, gs=0.25),
       "nesterov": dict(mom=f32(0.9), wd=0.0, nesterov=1, first=0, lr_dev=True, gs=None),
       "weight_decay": dict(mom=f32(0.9), wd=f32(1e-4), nesterov=0, first=0, lr_dev=False, gs=None)}


def _sgd(variant, n, off):
    hp = SGD[variant]
    p0, (g, b0) = _gen(R.gen_opt, n, steps=2)
    p, gd = _dev(p0, off), _dev(g, off)
    buf = None
    if hp["mom"]:
        buf = _out(n, off) if hp["first"] else _dev(b0, off)     # (the first step must not read its NaNs)
    lr_dev = torch.tensor([R.SGD_LR], device="cuda") if hp["lr_dev"] else None
    gs_dev = torch.tensor([hp["gs"]], device="cuda") if hp["gs"] is not None else None
    _ok(_lib.load().srk_sgd_step(P(p), P(gd), P(buf), n, 0.0 if hp["lr_dev"] else R.SGD_LR, hp["mom"], hp["wd"],
                                 hp["nesterov"], hp["first"], P(lr_dev), P(gs_dev), S()))
    return {"p": p, "buf": buf} if buf is not None else {"p": p}


for _v in SGD:
    for _tag, _n, _off in _forms(None, R.CAP_RED if _v in ("plain", "nesterov") else None):
        if _tag == "v1off" and _v != "weight_decay":
            continue
        case("sgd_%s_%s" % (_v, _tag))(lambda v=_v, n=_n, off=_off: _sgd(v, n, off))


# ---- Adam: two calls back to back, so the second reads the count and the cleared ticket the first left -----------------------
def _adam(wd, n, off):
    lr_on_dev, gs = (False, None) if wd == 0.0 else (True, 0.25)
    p0, grads = _gen(R.gen_opt, n, steps=2)
    z = np.zeros(n, np.float32)
    p, m, v = _dev(p0, off), _dev(z, off), _dev(z, off)
    step = torch.zeros(2, dtype=torch.int32, device="cuda")
    lr_dev = torch.tensor([R.ADAM["lr"]], device="cuda") if lr_on_dev else None
    gs_dev = torch.tensor([gs], device="cuda") if gs is not None else None
    for g in grads:
        gd = _dev(g, off)
        _ok(_lib.load().srk_adam_step(P(p), P(gd), P(m), P(v), n, 0.0 if lr_on_dev else R.ADAM["lr"], R.ADAM["b1"],
                                      R.ADAM["b2"], R.ADAM["eps"], wd, P(step), P(lr_dev), P(gs_dev), S()))
    return {"p": p, "m": m, "v": v, "step": step}


for _wd in (0.0, f32(1e-4)):
    for _tag, _n, _off in _forms(R.CAP_ADAM4, R.CAP_RED):
        if _tag.endswith("cap") and _wd == 0.0 or _tag == "v1off" and _wd == 0.0:
            continue
        case("adam_%s_%s" % ("wd" if _wd else "plain", _tag))(lambda wd=_wd, n=_n, off=_off: _adam(wd, n, off))


# ---- losses --------------------------------------------------------------------------------------------------------------
EPS = f32(1e-6)


def _loss(kind, dims, target="dense", off=0, grad=True):
    """pred NHWC-dense; target dense (NULL strides), one float off a 16-byte boundary, or NCHW through strides"""
    N, C, H, W = dims
    n = N * C * H * W
    p, t = _gen(lambda m: R.gen_loss(kind, m), n)
    pd = _dev(p)
    st = None
    if target == "nchw":     # t holds the logical [N, C, H, W] values in NCHW order
        td, st = _dev(t), (ctypes.c_int64 * 4)(C * H * W, H * W, W, 1)
        assert (N - 1) * st[0] + (C - 1) * st[1] + (H - 1) * st[2] + (W - 1) * st[3] == td.numel() - 1
    else:
        td = _dev(t, off)
    dp = _out(n) if grad else None
    out = _out(1)
    lib = _lib.load()
    _ok(lib.srk_loss_forward_backward(R.LOSSES.index(kind), P(pd), P(td), st, N, C, H, W, EPS if kind == "charbonnier" else 0.0,
                                      f32(0.25), P(out), P(dp), P(_ws(lib.srk_loss_workspace_bytes())), S()))
    return {"loss": out, "dpred": dp} if grad else {"loss": out}


for _k in R.LOSSES:
    for _tag, _n, _off in _forms(R.CAP_LOSS4, R.CAP_RED):
        if _tag.endswith("cap") and _k not in ("mse", "bce"):
            continue
        case("loss_%s_%s" % (_k, _tag))(lambda k=_k, n=_n, off=_off: _loss(k, (1, 1, 1, n), off=off))
    case("loss_%s_nchw" % _k)(lambda k=_k: _loss(k, (2, 3, 20, 21), "nchw"))
case("loss_mse_nchw_cap")(lambda: _loss("mse", (2, 3, 592, 592), "nchw"))
case("loss_l1_v4_value_only")(lambda: _loss("l1", (1, 1, 1, NV), grad=False))
case("loss_l1_v1_value_only")(lambda: _loss("l1", (1, 1, 1, NS), grad=False))


# ---- activations ---------------------------------------------------------------------------------------------------------
def _act(kind, n, off=0, C=1):
    """forward into y, then the backward from what the forward saved.  The single slope's gradient starts from zero and is
    kept only where at most two blocks add to it; the per-channel one is not kept."""
    x, dy = _gen(R.gen_act, n)
    w = {"prelu": R.gen_prelu_w(1), "prelu_c": R.gen_prelu_w(C)}.get(kind)
    xd, wd = _dev(x), (_dev(w) if w is not None else None)
    y = _out(n)
    lib = _lib.load()
    pn = 0 if w is None else w.size
    assert n % C == 0
    _ok(lib.srk_act_forward(P(xd), P(y), n, C, R.ACT_CODE[kind], f32(0.2), P(wd), pn, S()))
    saved = xd if w is not None else y
    dx = _out(n, off)
    dpw = torch.zeros(pn, device="cuda") if w is not None else None
    _ok(lib.srk_act_backward(P(_dev(dy)), P(saved), P(dx), n, C, R.ACT_CODE[kind], f32(0.2), P(wd), pn, P(dpw), S()))
    if kind == "prelu" and n <= 4096:
        return {"y": y, "dx": dx, "dprelu": dpw}
    return {"y": y, "dx": dx}


for _k in ("relu", "lrelu", "prelu", "tanh", "sigmoid"):
    for _tag, _n, _off in _forms(R.CAP_EW, R.CAP_EW):
        if _tag.endswith("cap") and _k not in (("lrelu", "prelu") if _tag == "v4cap" else ("relu", "tanh")):
            continue
        if _tag == "v1off" and _k not in ("relu", "prelu"):
            continue
        case("act_%s_%s" % (_k, _tag))(lambda k=_k, n=_n, off=_off: _act(k, n, off))
case("act_prelu_c6")(lambda: _act("prelu_c", 6 * 408, C=6))      # (!vec_ok forward branch; per-channel backward)
case("act_prelu_c8")(lambda: _act("prelu_c", 8 * 306, C=8))      # (four slopes per 16-byte group)


def _axpby(n):
    a, b = _gen(R.gen_act, n, seed=29)
    out = _out(n)
    _ok(_lib.load().srk_axpby(P(_dev(a)), P(_dev(b)), P(out), n, f32(0.3), f32(-1.7), S()))
    return {"out": out}


case("axpby_small")(lambda: _axpby(NS))
case("axpby_cap")(lambda: _axpby(R.CAP_EW + 3))


def _absmax(n, off):
    x = _gen(lambda m: R._rs(m % 1000).uniform(-0.5, 0.5, m).astype(np.float32), n)
    slots = torch.zeros(_lib.AMAX_FLOATS, device="cuda")
    _ok(_lib.load().srk_absmax(P(_dev(x, off)), n, P(slots), S()))
    return {"slots": slots}


case("absmax_aligned")(lambda: _absmax(2 * 4096 + 403, 0))
case("absmax_off1")(lambda: _absmax(2 * 4096 + 403, 1))
case("absmax_cap")(lambda: _absmax(R.CAP_ABSMAX + 3, 0))
case("absmax_cap_off1")(lambda: _absmax(R.CAP_ABSMAX + 3, 1))


def _pixel_shuffle(C, r):
    N, H, W = 2, 5, 7
    x = R.gen_act(N * H * W * C * r * r, seed=C + r)[0]
    y, dx = _out(x.size), _out(x.size)
    lib = _lib.load()
    _ok(lib.srk_pixel_shuffle_forward(P(_dev(x)), P(y), N, H, W, C, r, S()))
    _ok(lib.srk_pixel_shuffle_backward(P(y), P(dx), N, H, W, C, r, S()))
    return {"y": y, "dx": dx}


case("pixel_shuffle_c3_r2")(lambda: _pixel_shuffle(3, 2))       # (scalar x side, scalar y side)
case("pixel_shuffle_c16_r2")(lambda: _pixel_shuffle(16, 2))     # (16-byte accesses on both sides)


# ---- reductions through partials: gradient norm, PSNR, sum of squares -------------------------------------------------------
def _norm(n):
    g = _gen(R.gen_mass, n, R.positions(min(n, TILE), R.grid_red(min(n, TILE))))
    out = _out(2)
    lib = _lib.load()
    _ok(lib.srk_grad_norm_clip(P(_dev(g)), n, f32(0.4), P(out[0:]), P(out[1:]), P(_ws(lib.srk_grad_norm_workspace_bytes())), S()))
    return {"norm_scale": out}


case("grad_norm_small")(lambda: _norm(NS))
case("grad_norm_cap")(lambda: _norm(R.CAP_RED + 3))


def _psnr(n):
    gt = _gen(lambda m: R._rs(7).uniform(0.25, 0.75, m).astype(np.float32), n)
    pred = gt + _gen(R.gen_mass, n) * np.float32(0.25)
    out = _out(2)
    lib = _lib.load()
    st = (ctypes.c_int64 * 4)(n, 1, n, 1)
    _ok(lib.srk_psnr(P(_dev(pred)), st, P(_dev(gt)), st, 1, 1, 1, n, P(out[0:]), P(out[1:]), P(_ws(lib.srk_psnr_workspace_bytes())), S()))
    return {"psnr_mse": out}


case("psnr_small")(lambda: _psnr(NS))
case("psnr_cap")(lambda: _psnr(R.CAP_RED + 3))


def _sumsq(n, off=0):
    p = _gen(lambda m: R.gen_opt(m, steps=0)[0], n)
    out = _out(1)
    lib = _lib.load()
    _ok(lib.srk_sumsq(P(_dev(p, off)), n, f32(0.5e-4), P(out), P(_ws(lib.srk_sumsq_workspace_bytes())), S()))
    return {"out": out}


for _tag, _n, _off in _forms(R.CAP_LOSS4, 1024 * 256):      # (one group of V floats per thread and pass, 1024 blocks)
    case("sumsq_%s" % _tag)(lambda n=_n, off=_off: _sumsq(n, off))


# ---- SSIM and the SSIM loss: the finals behind a few blocks and behind the saturated partial count (8192) -----------------
def _images(N, C, H, W, seed):
    n = N * C * H * W
    gt = _gen(lambda m: R._rs(seed).uniform(0.0, 1.0, m).astype(np.float32), n)
    return gt + _gen(R.gen_mass, n, seed=seed + 1) * np.float32(20.0), gt, n


def _ssim(N, C, H, W):
    pred, gt, n = _images(N, C, H, W, 31)
    out = _out(3)
    lib = _lib.load()
    _ok(lib.srk_ssim(P(_dev(pred)), None, P(_dev(gt)), None, N, C, H, W, 0, 0, P(out[0:]), P(out[1:]), P(out[2:]),
                     P(_ws(lib.srk_ssim_workspace_bytes())), S()))
    return {"ssim_psnr_mse": out}


case("ssim_small")(lambda: _ssim(1, 3, 30, 150))              # 3 x 3 tiles of 8 x 64 positions
case("ssim_cap")(lambda: _ssim(1, 1, 10 + 8 * 130, 10 + 64 * 64))      # 130 x 64 = 8320 tiles > 8192


def _ssim_loss(N, C, H, W):
    pred, gt, n = _images(N, C, H, W, 37)
    out, dp = _out(1), _out(n)
    lib = _lib.load()
    _ok(lib.srk_ssim_loss_forward_backward(P(_dev(pred)), P(_dev(gt)), None, N, C, H, W, f32(0.25), P(out), P(dp),
                                           P(_ws(lib.srk_ssim_loss_workspace_bytes())), S()))
    return {"loss": out, "dpred": dp}


case("ssim_loss_small")(lambda: _ssim_loss(1, 3, 30, 37))     # 2 x 3 tiles of 16 x 16 pixels
case("ssim_loss_cap")(lambda: _ssim_loss(1, 1, 16 * 91 + 3, 16 * 91))      # 92 x 91 = 8372 tiles > 8192


# ---- DRCN head -------------------------------------------------------------------------------------------------------------
def _drcn(M, off, D=3, backward=False):
    y = _gen(lambda m: R.gen_act(m, seed=43)[1], D * M)
    x, t = _gen(lambda m: R.gen_loss("mse", m), M)
    w = (np.arange(D, dtype=np.float32) + 1) / np.float32(D) + np.float32(0.1)
    Y, wd = _dev(y, off), _dev(w)
    lib = _lib.load()
    nws = int(lib.srk_drcn_workspace_bytes(D))
    dY = _out(D * M, off)
    dw = torch.full((D,), 0.75, device="cuda")
    if backward:
        dout = _gen(lambda m: R.gen_act(m, seed=47)[1], M)
        _ok(lib.srk_drcn_head_backward(P(Y), P(wd), P(_dev(dout, off)), D, 1, 1, 1, M, P(dY), P(dw), f32(0.5), P(_ws(nws)), nws, S()))
        return {"dY": dY, "dw": dw}
    alpha, reg = torch.tensor([0.3], device="cuda"), torch.tensor([0.0625], device="cuda")
    out, loss, terms = _out(M, off), _out(1), _out(2)
    _ok(lib.srk_drcn_head_loss(P(Y), P(_dev(x, off)), P(_dev(t, off)), P(wd), D, 1, 1, 1, M, P(alpha), P(reg), f32(0.25), P(out),
                               P(dY), P(loss), P(terms), P(dw), 0.0, P(_ws(nws)), nws, S()))
    return {"out": out, "dY": dY, "loss": loss, "terms": terms, "dw": dw}


# (one group of V floats per thread and pass, at most 1024 blocks: three blocks are 612 groups)
for _tag, _m, _off in (("v4", NV, 0), ("v1", 611, 0), ("v1off", 612, 1), ("v4cap", R.CAP_LOSS4 + 4, 0), ("v1cap", 1024 * 256 + 3, 0)):
    case("drcn_loss_%s" % _tag)(lambda m=_m, off=_off: _drcn(m, off))
    case("drcn_backward_%s" % _tag)(lambda m=_m, off=_off: _drcn(m, off, backward=True))
case("drcn_loss_d5_v4")(lambda: _drcn(NV, 0, D=5))      # (the 16-deep instantiation)


# ---- nearest up-sampling, 2x2 max-pool backward -----------------------------------------------------------------------------
def _upsample(C, H, W):
    x = _gen(lambda m: R.gen_act(m, seed=C)[0], H * W * C)
    y = _out(H * 2 * W * 2 * C)
    _ok(_lib.load().srk_upsample_nearest_forward(P(_dev(x)), P(y), 1, H, W, C, 2, S()))
    return {"y": y}


case("upsample_c4")(lambda: _upsample(4, 15, 21))             # 1260 groups: three blocks of 512
case("upsample_c3")(lambda: _upsample(3, 15, 21))             # 3780 floats: four blocks of 1024
case("upsample_c4_cap")(lambda: _upsample(4, 1025, 512))
case("upsample_c3_cap")(lambda: _upsample(3, 592, 592))


def _maxpool_bwd(C, H, W, relu_input, N=2):
    x = _gen(lambda m: R.gen_act(m, seed=C + H)[0], N * H * W * C)
    dy = _gen(lambda m: R.gen_act(m, seed=C + W)[1], N * (H // 2) * (W // 2) * C)
    dx = _out(x.size)
    _ok(_lib.load().srk_maxpool2x2_backward(P(_dev(x)), P(_dev(dy)), P(dx), N, H, W, C, relu_input, S()))
    return {"dx": dx}


for _c in (3, 8):
    case("maxpool_bwd_c%d" % _c)(lambda c=_c: _maxpool_bwd(c, 15, 21, 0))      # 2 x 8 x 11 windows: two blocks either form
    case("maxpool_bwd_c%d_relu" % _c)(lambda c=_c: _maxpool_bwd(c, 15, 21, 1))
case("maxpool_bwd_c3_cap")(lambda: _maxpool_bwd(3, 1673, 1673, 1, N=1))        # 837^2 x 3 > 4096 x 512 items
case("maxpool_bwd_c8_cap")(lambda: _maxpool_bwd(8, 1449, 1449, 1, N=1))        # 725^2 x 2 > 4096 x 256 groups

NAMES = sorted(CASES)


# ---- comparison ------------------------------------------------------------------------------------------------------------
def run_case(name):
    """{key: numpy array of the raw 32-bit words}"""
    out = {}
    try:
        for k, v in CASES[name]().items():
            a = np.ascontiguousarray(v.detach().cpu().numpy()).reshape(-1)
            assert a.dtype.itemsize == 4
            out[k] = a.view(np.uint32)
    finally:
        torch.cuda.synchronize()
        del _KEEP[:]
    return out


def corner(a):
    return np.ascontiguousarray(a[-CORNER:])


def digest(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


@pytest.fixture(scope="module")
def hashes():
    with open(os.path.join(GOLDEN, "sha256.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", NAMES)
def test_bit_identical_to_parent(gpu, hashes, name):
    got = run_case(name)
    want = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    assert set(got) == {k[:-len("_corner")] if k.endswith("_corner") else k for k in want.files}
    for k, a in got.items():
        if a.nbytes <= WHOLE_BYTES:
            assert a.shape == want[k].shape and want[k].dtype == np.uint32
            assert np.array_equal(a, want[k]), "%s: %d of %d words differ" % (k, int((a != want[k]).sum()), a.size)
        else:
            assert np.array_equal(corner(a), want[k + "_corner"]), k + " corner"
            assert digest(a) == hashes[name][k], k
