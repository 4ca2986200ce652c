"""autograd.Function wrappers around the C ABI (include/srk.h).

Every function here enqueues hand-written HIP kernels on torch's current stream and returns
torch tensors that merely OWN the device memory.  Activations are logically NCHW (the reference's
module surface, e.g. edsr.py:146-152) but stored channels_last (= dense NHWC, the kernels'
layout).  Nothing in this file computes on the CPU and nothing falls back to ATen operators.
"""
import collections
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import (ACT_BY_NAME, ACT_LRELU, ACT_NONE, ACT_PRELU, ACT_RELU, ALGO_AUTO, BwdMask, ConvDesc, Epilogue,
                   check, ptr, require_cuda, stream_ptr)

CL = torch.channels_last

# Convolution arithmetic used when a ConvCfg leaves algo = AUTO, per role:
#   infer     forward under torch.no_grad()
#   train_fwd forward that will be differentiated
#   bwd       data gradient
# Modes:
#   "mixed"  (default; round 3: infer = the fp32-faithful class too -- f16x3 costs ~10 % over bf16x3 on the c2 net, and a
#            drop-in for an fp32 reference should not default to narrower products; "bf16x3" is the fast option)
#            train_fwd = fp32-faithful class: f16x3 where it pays, else bf16x6 (exact 3-way operand split, 6 bf16 MFMAs per
#            product: measured 3.5e-7 rms / 8.8e-7 max error vs fp64 — tighter than the fp32 MFMA
#            kernel's 4.3e-7 / 1.2e-6 — at 1.5-2x its speed; shapes it does not cover run exact fp32),
#            bwd = bf16x3.  The training forward stays fp32-faithful so that ReLU / LeakyReLU masks are
#            decided on fp32-accurate values (a 5e-6 forward perturbation flips ~1e-5 of the units of
#            a bias-free ReLU net, and one flipped unit moves that layer's gradient by
#            ~1/sqrt(units) ~ 1e-2); gradients then only carry the ~5e-6 arithmetic error of the
#            bf16x3 data-gradient kernels.
#            train_fwd_tail = bf16x3: the training forward of the layers a model marks `_linear_tail` -- nothing
#            but convolutions, additions and pixel shuffles between their output and the loss (EDSR: body-end conv,
#            the two upsampler convs, the reconstruction conv; VDSR: the reconstruction conv), so no mask depends on
#            their rounding and the ~5e-6 of the backward kernels is what their forward may carry as well (EDSR step
#            7.11 -> 6.67 ms).  "bf16x6" keeps the fp32-faithful products there too; LINEAR_TAIL_X3 = False likewise.
#   "bf16x3" everything on the 3-term bf16 split (fastest; forward error ~1e-5, gradients subject to
#            the mask-flip sensitivity above).
#   "fp32"   everything exact fp32 (summation-order-level agreement with ATen/oneDNN).
_MODES = {"mixed": {"infer": _lib.ALGO_MFMA_BF16X6, "train_fwd": _lib.ALGO_MFMA_BF16X6, "bwd": ALGO_AUTO,
                    "train_fwd_tail": ALGO_AUTO},
          # fp32-faithful products everywhere they exist (inference included): what "mixed" costs when bf16x3's ~5e-6 is
          # not acceptable for the forward either
          "bf16x6": {"infer": _lib.ALGO_MFMA_BF16X6, "train_fwd": _lib.ALGO_MFMA_BF16X6, "bwd": ALGO_AUTO,
                     "train_fwd_tail": _lib.ALGO_MFMA_BF16X6},
          # ... and in both gradient kernels too (data gradient on the six-MFMA split, weight gradient on the exact fp32 MFMA
          # kernels): every product of a train step at fp32 accuracy -- the reference point for what the 3-MFMA backward costs
          "faithful": {"infer": _lib.ALGO_MFMA_BF16X6, "train_fwd": _lib.ALGO_MFMA_BF16X6, "bwd": _lib.ALGO_MFMA_BF16X6,
                       "train_fwd_tail": _lib.ALGO_MFMA_BF16X6},
          "bf16x3": {"infer": ALGO_AUTO, "train_fwd": ALGO_AUTO, "bwd": ALGO_AUTO, "train_fwd_tail": ALGO_AUTO},
          "fp32": {"infer": _lib.ALGO_MFMA, "train_fwd": _lib.ALGO_MFMA, "bwd": _lib.ALGO_MFMA,
                   "train_fwd_tail": _lib.ALGO_MFMA}}
_PRECISION = {"mode": "mixed"}


def set_precision(mode):
    """Select the convolution arithmetic: 'mixed' (default), 'bf16x3', 'bf16x6', 'faithful' or 'fp32' (see above)."""
    if mode not in _MODES:
        raise ValueError("precision must be one of %s" % sorted(_MODES))
    _PRECISION["mode"] = mode


def get_precision():
    return _PRECISION["mode"]


def backward_arithmetic():
    """What the data- and weight-gradient products run on in the current mode (bench.py states it next to every training
    number)."""
    mode = _PRECISION["mode"]
    if mode == "fp32":
        return "exact fp32 MFMA"
    if mode == "faithful":
        return "bf16x6 data gradients (6 MFMAs, ~3e-7 rms), exact fp32 MFMA weight gradients"
    return "bf16x3 (3 MFMAs, ~5e-6 rms)"


def _algo_for(cfg, role):
    return cfg.algo if cfg.algo != ALGO_AUTO else _MODES[_PRECISION["mode"]][role]


# ------------------------------------------------------------------------------------------------
# fp32-faithful products with three MFMAs: SRK_ALGO_MFMA_F16X3
# ------------------------------------------------------------------------------------------------
# Wherever a mode asks for the fp32-faithful class (ALGO_MFMA_BF16X6: six bf16 MFMAs per product) and the fp16 kernels
# cover the layer, the forward runs f16x3 instead: both operands scaled by a power of two so that their largest magnitude
# sits at 2^13..2^14, split into two fp16 planes (2 x 11 bits), three MFMAs, exact descale -- 1.2e-7 rms against 0.8e-7
# for plain fp32 products and 7.6e-8 for bf16x6 (tools/precision_check.py), at the bf16x3 rate.  The scale of the
# activations needs an upper bound of max|x| ON THE DEVICE: every kernel that can (conv_bfd.hip, conv_res2.hip) leaves
# the running maximum of what it stored in a 1 KB buffer of 16 slots (`y_amax`), attached to the output tensor as `_srk_amax`;
# tensors without one (network inputs, outputs of other kernels) get it from one srk_absmax pass.  SRK_F16X3=0: off.
F16X3 = os.environ.get("SRK_F16X3", "1") != "0"
F16X3_ALWAYS = os.environ.get("SRK_F16X3", "1") == "2"   # tests: take the srk_absmax pass for every untagged input
_AMAX_CHUNK_TENSORS = 128
_AMAX = {}   # device index -> [chunk tensor, slots used]
_AMAX_EPOCH = [0]


def amax_new_step(chunk=None):
    """Start of a train step (optimizer.zero_grad) or of a graph capture: the next running maximum comes from a fresh
    zeroed chunk (inside a captured step the zero fill is part of the graph, so every replay starts from zero), and
    maxima attached to tensors before this point are no longer trusted -- a captured step must recompute the maximum of
    its static input buffers inside the graph, where every replay sees the batch of that replay.
    chunk: a float32 tensor of a multiple of AMAX_FLOATS elements that the CALLER zeroes on the stream before the step's
    first kernel (optim.FlatParams keeps one next to its gradients: one fill for both); the step's first buffers come
    from it, further ones from chunks allocated (and zeroed) here."""
    _AMAX.clear()
    _AMAX_EPOCH[0] += 1
    if chunk is not None:
        idx = chunk.device.index if chunk.device.index is not None else torch.cuda.current_device()
        _AMAX[idx] = [chunk, 0, chunk.numel() // _lib.AMAX_FLOATS]


def _amax_alloc(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ent = _AMAX.get(idx)
    if ent is None or ent[1] >= ent[2]:
        ent = _AMAX[idx] = [torch.zeros(_AMAX_CHUNK_TENSORS * _lib.AMAX_FLOATS, dtype=torch.float32,
                                        device=torch.device("cuda", idx)), 0, _AMAX_CHUNK_TENSORS]
    lo = ent[1] * _lib.AMAX_FLOATS
    ent[1] += 1
    return ent[0][lo:lo + _lib.AMAX_FLOATS]


F16X3_MIN_PIXELS = int(os.environ.get("SRK_F16X3_MIN_PIXELS", str(256 * 2 * 256)))


def _f16x3_pays(d):
    """Where three MFMAs instead of six are worth the running-maximum bookkeeping: problems large enough to be bound by
    the matrix work (conv_bfd.hip's large-block configurations: >= two 256-pixel tiles per CU; first layers of that size
    leave the fp32 MFMA kernel for the row-packed one) and kernels with more than nine taps.  The 64-pixel blocks of a small 3x3
    problem are a latency chain -- measured on the SRGAN step (16 patches): 18.7 us with f16x3 against 19.1 us with
    bf16x6 per conv, and the maxima cost more than that."""
    return (d.KH * d.KW > 9 or F16X3_ALWAYS
            or d.N * d.OH * d.OW * ((d.Cout + 63) // 64) >= F16X3_MIN_PIXELS)


def _ver(t):
    """Version counter of `t` for the "unchanged since it was tagged" tests below.  Tensors created under
    torch.inference_mode() track none (reading `_version` raises): the constant stands in, i.e. a tag on an inference
    tensor is trusted for the tensor's lifetime -- nothing in this package writes an activation in place."""
    return -1 if t.is_inference() else t._version


def _tag_amax(t, slots):
    t._srk_amax = (slots, _ver(t), _AMAX_EPOCH[0])


def amax_of(x, compute=True):
    """The running-maximum buffer of |x| on the device: the producer's, or one srk_absmax pass.  compute=False: only
    where that pass is known to pay -- x carries the marker a conv kernel without amax support leaves on its output
    (the first layer of a net: one pass buys f16x3 for the whole trunk behind it); anything else (a BatchNorm output in
    front of every SRGAN conv) returns None and the caller keeps the six-MFMA arithmetic."""
    a = getattr(x, "_srk_amax", None)
    fresh = a is not None and a[1] == _ver(x) and a[2] == _AMAX_EPOCH[0]
    if fresh and a[0] is not None:
        return a[0]
    if not compute and not fresh:
        return None
    slots = _amax_alloc(x.device)
    xs = x if x.is_contiguous() or _is_nhwc_dense(x) else x.contiguous()
    check(_lib.load().srk_absmax(ptr(xs), xs.numel(), ptr(slots), stream_ptr()), "srk_absmax")
    try:
        _tag_amax(x, slots)
    except Exception:  # noqa: BLE001 -- (a tensor subclass without a __dict__: recomputed next time)
        pass
    return slots


_BOUND_SLOTS = {}   # (device index, bound) -> slots filled with the bound: no kernel runs for a declared maximum


def declare_absmax(x, bound):
    """The caller's promise that |x| <= bound everywhere (e.g. 1.0 for a ToTensor image batch, dataset.py:71): the
    fp32-faithful f16x3 kernels then scale x by that bound and the srk_absmax pass over x is not run.  The C ABI asks for
    slots whose maximum is >= max|x| (include/srk.h, srk_epilogue.x_amax), so a true bound is as good as the maximum (a loose
    one costs mantissa bits of the 22 the two fp16 planes hold: 2^-k of them for a bound 2^k too large); a FALSE one lets the
    scaled fp16 planes overflow to inf.  Returns x, tagged."""
    require_cuda(x)
    idx = x.device.index if x.device.index is not None else torch.cuda.current_device()
    key = (idx, float(bound))
    slots = _BOUND_SLOTS.get(key)
    if slots is None:
        slots = _BOUND_SLOTS[key] = torch.full((_lib.AMAX_FLOATS,), float(bound), dtype=torch.float32,
                                               device=torch.device("cuda", idx))
    _tag_amax(x, slots)
    return x


def _empty_cl(n, c, h, w, like):
    return torch.empty((n, c, h, w), dtype=torch.float32, device=like.device, memory_format=CL)


def _is_nhwc_dense(x):
    """Memory is dense NHWC (strides of size-1 dims are irrelevant — views may rewrite them)."""
    n, c, h, w = x.shape
    want = (h * w * c, 1, w * c, c)
    return all(sz == 1 or st == e for sz, st, e in zip(x.shape, x.stride(), want))


def _is_nchw_dense(x):
    n, c, h, w = x.shape
    want = (c * h * w, h * w, w, 1)
    return all(sz == 1 or st == e for sz, st, e in zip(x.shape, x.stride(), want))


def to_nhwc(x):
    """Logical NCHW tensor -> same values, channels_last storage (srk_nchw_to_nhwc if a copy is needed)."""
    require_cuda(x)
    if x.dim() != 4:
        raise RuntimeError("expected a 4-D NCHW tensor, got shape %s" % (tuple(x.shape),))
    if _is_nhwc_dense(x):
        return x
    n, c, h, w = x.shape
    if not _is_nchw_dense(x):
        raise RuntimeError("input must be NCHW-contiguous or channels_last (got strides %s)" % (x.stride(),))
    y = _empty_cl(n, c, h, w, x)
    lib = _lib.load()
    check(lib.srk_nchw_to_nhwc(ptr(x), ptr(y), n, c, h, w, stream_ptr()), "srk_nchw_to_nhwc")
    a = getattr(x, "_srk_amax", None)   # a permutation keeps the maximum (or the "worth a pass" marker)
    if a is not None and a[1] == _ver(x) and a[2] == _AMAX_EPOCH[0]:
        _tag_amax(y, a[0])
    return y


# ---- pre-masked gradients ---------------------------------------------------------------------------------------------
# A conv with a fused ReLU multiplies its incoming dy by (y > 0) in BOTH backward kernels, reading y twice more.  When the
# consumer of y is another conv whose data gradient runs on the wave-specialised kernel, that kernel applies the mask to
# the dx it writes instead (srk_conv2d_backward_data_relu: y is its own input x, read once at the output tile) and marks
# the tensor: `_srk_premasked = (address of y, version of dx)`.  The upstream backward skips its masks only if the
# gradient it receives carries the mark for ITS y and is untouched since (autograd's fan-in accumulation adds in place
# and bumps the version; a fresh sum carries no mark).  ReLU only: its 0/1 mask is idempotent, so a mark that got lost
# merely costs the second application.  PREMASK = False switches the protocol off.
# The gradient of an INTERMEDIATE activation is not what autograd defines while the protocol runs (it is already
# multiplied by the ReLU gradient of its producer), so the protocol is active only inside `premasked_gradients()` -- the
# backward passes of this package's own training steps (trainers._backward), where only parameter gradients are read.
# A plain loss.backward(), torch.autograd.grad(loss, activation) or tensor.retain_grad() outside it sees standard gradients.
PREMASK = True
PREMASK_STATS = {"masked_dx": 0, "masks_skipped": 0}   # (tests: how often each half of the protocol ran)
_PREMASK_DEPTH = [0]


class premasked_gradients(object):
    """Backward passes inside this context may hand pre-masked gradients from layer to layer (see PREMASK)."""

    def __enter__(self):
        _PREMASK_DEPTH[0] += 1
        return self

    def __exit__(self, *a):
        _PREMASK_DEPTH[0] -= 1


def _premask_on():
    return PREMASK and _PREMASK_DEPTH[0] > 0


def _is_relu_output(x):
    return getattr(x, "_srk_relu_out", None) == _ver(x)


def _premasked_for(dy, y):
    t = getattr(dy, "_srk_premasked", None)
    return _premask_on() and t is not None and t == (y.data_ptr(), _ver(dy))


def to_nchw(x):
    """channels_last tensor -> NCHW-contiguous copy (srk_nhwc_to_nchw). Used before Linear layers."""
    require_cuda(x)
    n, c, h, w = x.shape
    if _is_nchw_dense(x):
        return x if x.is_contiguous() else x.contiguous()
    x = to_nhwc(x)
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    check(lib.srk_nhwc_to_nchw(ptr(x), ptr(y), n, c, h, w, stream_ptr()), "srk_nhwc_to_nchw")
    return y


class _ToNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return to_nchw(x)

    @staticmethod
    def backward(ctx, g):
        return to_nhwc(g if (_is_nchw_dense(g) or _is_nhwc_dense(g)) else g.contiguous())


def flatten_nchw(x):
    """out.view(B, -1) of the reference (srgan.py:75) — flatten in (C,H,W) order."""
    y = _ToNCHW.apply(x)
    return y.reshape(y.shape[0], -1)


# ------------------------------------------------------------------------------------------------
# Convolution
# ------------------------------------------------------------------------------------------------
class ConvCfg(object):
    """Static configuration of one Conv2d / ConvTranspose2d call."""
    __slots__ = ("stride", "pad", "transposed", "out_pad", "act", "slope", "ps_r", "algo", "tail")

    def __init__(self, stride=1, pad=0, transposed=False, out_pad=0, act=ACT_NONE, slope=0.0, ps_r=0,
                 algo=ALGO_AUTO):
        self.stride, self.pad, self.transposed, self.out_pad = int(stride), int(pad), bool(transposed), int(out_pad)
        self.act, self.slope, self.ps_r, self.algo = int(act), float(slope), int(ps_r), int(algo)
        self.tail = False   # training forward of a layer with no nonlinearity between its output and the loss


def _weight_dims(weight, transposed):
    if transposed:
        cin, cout, kh, kw = weight.shape
    else:
        cout, cin, kh, kw = weight.shape
    return cout, cin, kh, kw


def _make_desc(x_shape, weight, cfg, role="infer"):
    lib = _lib.load()
    n, c, h, w = x_shape
    cout, cin, kh, kw = _weight_dims(weight, cfg.transposed)
    if c != cin:
        raise RuntimeError("conv: input has %d channels, weight expects %d" % (c, cin))
    oh = lib.srk_conv_out_dim(h, kh, cfg.stride, cfg.pad, int(cfg.transposed), cfg.out_pad)
    ow = lib.srk_conv_out_dim(w, kw, cfg.stride, cfg.pad, int(cfg.transposed), cfg.out_pad)
    if oh <= 0 or ow <= 0:
        raise RuntimeError("conv: empty output for input %s kernel %dx%d" % (tuple(x_shape), kh, kw))
    algo = _algo_for(cfg, role)
    return ConvDesc(n, h, w, cin, oh, ow, cout, kh, kw, cfg.stride, cfg.pad, int(cfg.transposed), cfg.out_pad, algo)


def pack_weight_fwd(weight, transposed, ps_r):
    lib = _lib.load()
    cout, cin, kh, kw = _weight_dims(weight, transposed)
    nbytes = int(lib.srk_packed_weight_bytes(cout, cin, kh, kw, 0))
    wp = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=weight.device)
    check(lib.srk_pack_weight_fwd(ptr(weight), ptr(wp), cout, cin, kh, kw, int(transposed), int(ps_r), stream_ptr()),
          "srk_pack_weight_fwd")
    return wp


def pack_weight_bwd(weight, transposed, ps_r=0):
    lib = _lib.load()
    cout, cin, kh, kw = _weight_dims(weight, transposed)
    nbytes = int(lib.srk_packed_weight_bytes(cout, cin, kh, kw, 1))
    wp = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=weight.device)
    check(lib.srk_pack_weight_bwd(ptr(weight), ptr(wp), cout, cin, kh, kw, int(transposed), int(ps_r), stream_ptr()),
          "srk_pack_weight_bwd")
    return wp


def pack_bias_ps(bias, ps_r):
    if bias is None or ps_r <= 1:
        return bias
    lib = _lib.load()
    bp = torch.empty_like(bias)
    check(lib.srk_pack_bias_ps(ptr(bias), ptr(bp), bias.numel(), int(ps_r), stream_ptr()), "srk_pack_bias_ps")
    return bp


# BatchNorm column sums from the producing conv's epilogue (srk_epilogue.bn_partial): a block that runs conv -> BatchNorm
# in training asks for them around the conv call; a kernel that keeps them (k_c64: the per-tile 64 -> 64 3x3 kernel of
# SRGAN's generator) tags its output, and _BatchNorm.forward then skips its own pass over the activation.
BN_PARTIAL = True
_BN_REQ = [0]


class bn_partial_request(object):
    """with ops.bn_partial_request(on): y = conv.run(x)   -- y may carry `_srk_bn_partial` afterwards"""

    def __init__(self, on=True):
        self.on = bool(on) and BN_PARTIAL

    def __enter__(self):
        if self.on:
            _BN_REQ[0] += 1
        return self

    def __exit__(self, *exc):
        if self.on:
            _BN_REQ[0] -= 1
        return False


def conv_forward_raw(x, wp, bias_p, weight_shape_src, cfg, prelu_w=None, residual=None, role="infer", x_nchw=False,
                     out=None):
    """Launch srk_conv2d_forward on already-packed weights. x must be NHWC-dense (or NCHW with x_nchw).
    out: an NHWC-dense tensor of the output's shape to write into (e.g. one slice of a stacked buffer); default: a new
    one."""
    lib = _lib.load()
    d = _make_desc(x.shape, weight_shape_src, cfg, role)
    d.x_nchw = int(bool(x_nchw))
    r = cfg.ps_r if cfg.ps_r > 1 else 1
    if out is None:
        y = _empty_cl(d.N, d.Cout // (r * r), d.OH * r, d.OW * r, x)
    else:
        want = (d.N, d.Cout // (r * r), d.OH * r, d.OW * r)
        if tuple(out.shape) != want or not _is_nhwc_dense(out) or out.dtype != torch.float32 or out.device != x.device:
            raise RuntimeError("conv: out= must be a dense NHWC fp32 tensor of shape %s on %s (got %s, strides %s)"
                               % (want, x.device, tuple(out.shape), out.stride()))
        y = out
    if residual is not None and tuple(residual.shape) != tuple(y.shape):
        raise RuntimeError("conv: residual shape %s != output shape %s" % (tuple(residual.shape), tuple(y.shape)))
    ep = Epilogue(ptr(bias_p), ptr(prelu_w), ptr(residual), cfg.slope, cfg.act,
                  0 if prelu_w is None else prelu_w.numel(), cfg.ps_r, None, None, None)
    bnp = None
    if (_BN_REQ[0] > 0 and role != "infer" and d.Cin == 64 and d.Cout == 64 and d.KH == 3 and d.KW == 3 and r == 1
            and cfg.act == ACT_NONE):
        # (the shape k_c64 covers; whether THAT kernel runs is the library's decision -- asked after the call)
        bnp = torch.empty((d.N * ((d.OH + 7) // 8) * ((d.OW + 7) // 8), 2 * d.Cout), dtype=torch.float64, device=x.device)
        ep.bn_partial = ptr(bnp)
    ya = None
    if d.algo == _lib.ALGO_MFMA_F16X3:      # asked for by name (ConvCfg.algo): the maximum is computed if nobody left one
        ep.x_amax = ptr(amax_of(x))
        ya = _amax_alloc(y.device)
        ep.y_amax = ptr(ya)
    elif F16X3 and d.Cout >= 8 and (d.Cin >= 8 or d.Cin <= 4) and _f16x3_pays(d):
        # fp32-faithful class on a layer the fp16 kernels cover: three MFMAs per product instead of six
        if d.algo == _lib.ALGO_MFMA_BF16X6 and lib.srk_conv2d_f16x3_supported(ctypes.byref(d), ctypes.byref(ep), ptr(y)):
            # (a first layer's input is the network input: one pass over a <= 4-channel tensor)
            xa = amax_of(x, compute=F16X3_ALWAYS or d.Cin <= 4)
            if xa is not None:
                ep.x_amax = ptr(xa)
                d.algo = _lib.ALGO_MFMA_F16X3
        if d.algo in (_lib.ALGO_MFMA_F16X3, _lib.ALGO_MFMA_BF16X6) and not os.environ.get("SRK_NO_YAMAX"):
            # (a layer of the fp32-faithful class feeds layers of that class: leave them the maximum of the output)
            ya = _amax_alloc(y.device)      # filled by the kernels of conv_bfd.hip (checked below)
            ep.y_amax = ptr(ya)
    if d.x_nchw and d.algo not in (ALGO_AUTO, _lib.ALGO_MFMA_BF16X3, _lib.ALGO_MFMA_F16X3):
        x = to_nhwc(x)      # only the bf16x3 / f16x3 first-layer kernels read an NCHW input in place
        d.x_nchw = 0
    # what the dispatched kernel did comes back in a host struct of the caller's (srk_conv_result)
    res = _lib.ConvResult()
    check(lib.srk_conv2d_forward_ex(ctypes.byref(d), ptr(x), ptr(wp), ptr(y), ctypes.byref(ep), ctypes.byref(res), stream_ptr()),
          "srk_conv2d_forward")
    if bnp is not None:
        rows_p = int(res.bn_partial_rows)
        if rows_p > 0:
            y._srk_bn_partial = (bnp, rows_p, _ver(y))
    if ya is not None and res.wrote_amax:
        _tag_amax(y, ya)
    elif F16X3 and d.algo in (_lib.ALGO_MFMA, _lib.ALGO_MFMA_BF16X6):
        _tag_amax(y, None)   # a faithful-class conv whose kernel leaves no maximum: worth one srk_absmax pass downstream
    return y


# ------------------------------------------------------------------------------------------------
# Deferred, grouped weight gradients
# ------------------------------------------------------------------------------------------------
# The data-gradient chain (layer L's dx feeds layer L-1) is the critical path of a backward pass; a layer's WEIGHT
# gradient feeds nothing until the optimizer / the gradient exchange.  In flat-buffer mode (optim.FlatParams: kernels
# accumulate straight into the flat gradient buffer, autograd never sees dw) the conv backward therefore only RECORDS
# (x, dy, mask) and the weight gradients of a whole backward pass are launched afterwards, grouped by geometry:
# srk_conv2d_backward_weight_grouped runs e.g. the 33 body convs of EDSR as ONE launch + one reduce launch in which every
# block walks ~40 tiles of one layer, instead of 66 launches of one-tile blocks that each write a 73 KB partial slab
# (strong-scaled shard of 16 patches: 0.89 ms -> 0.1x of the step).  The flush happens at the end of the backward pass
# (autograd engine callback) — `loss.backward(); p.grad` keeps working — or, under data parallelism, group by group
# from dp.DataParallel.exchange(), which sends each group's bucket off while the next group computes.
DEFER_WGRAD = True
# Deferral trades launches and partial-slab traffic for cache locality: a weight gradient launched right behind its
# layer's data gradient finds dy (and x) in the 256 MB Infinity Cache, one launched at the end of the pass reads them
# from HBM.  Records are therefore flushed (grouped) as soon as their x + dy bytes exceed DEFER_MAX_BYTES: a 16-patch
# EDSR shard (8 MB per layer) defers ~19 layers at a time, a 128-patch batch (67 MB per layer) falls back to
# one-or-two-layer groups, i.e. the per-layer behaviour.
DEFER_MAX_BYTES = 160 << 20
WgradRecord = collections.namedtuple("WgradRecord", "key desc x dy mask_y slope dw db")
_PENDING = []                      # WgradRecords in backward order (dw / db: views of the flat gradient buffer)
_DEFER = {"queued": False, "manual": 0, "bytes": 0}


class manual_wgrad_flush(object):
    """Context: the end-of-backward callback leaves the recorded weight gradients pending; the caller flushes them
    (flush_wgrads) — used by the trainers to interleave the grouped launches with the gradient exchange."""

    def __enter__(self):
        _DEFER["manual"] += 1

    def __exit__(self, *a):
        _DEFER["manual"] -= 1


def _auto_flush():
    _DEFER["queued"] = False
    if not _DEFER["manual"]:
        flush_wgrads()


def pending_wgrad_groups(max_layers=None):
    """The recorded weight gradients as launch groups [[record, ...], ...]: same geometry (and bias / no bias), backward
    order, no two records of a group writing the same dw (shared weights), at most `max_layers` layers per group."""
    cap = max_layers or 0
    groups, open_by_key = [], {}
    for rec in _PENDING:
        key, wptr = rec.key, rec.dw.data_ptr()
        g = open_by_key.get(key)
        if g is None or wptr in g[1] or (cap and len(g[0]) >= cap):
            g = ([], set())
            groups.append(g)
            open_by_key[key] = g
        g[0].append(rec)
        g[1].add(wptr)
    return [g[0] for g in groups]


def launch_wgrad_group(recs):
    """One srk_conv2d_backward_weight_grouped call for records of one geometry (beta = 1: accumulate into the flat
    gradient views)."""
    lib = _lib.load()
    n = len(recs)
    d = recs[0].desc
    vp = ctypes.c_void_p
    xs = (vp * n)(*[r.x.data_ptr() for r in recs])
    dys = (vp * n)(*[r.dy.data_ptr() for r in recs])
    masks = (BwdMask * n)(*[BwdMask(None if r.mask_y is None else r.mask_y.data_ptr(), r.slope) for r in recs])
    dws = (vp * n)(*[r.dw.data_ptr() for r in recs])
    has_bias = recs[0].db is not None
    dbs = (vp * n)(*[r.db.data_ptr() for r in recs]) if has_bias else None
    dev = recs[0].dy.device
    ws_bytes = int(lib.srk_conv2d_backward_weight_grouped_workspace_bytes(ctypes.byref(d), n))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    check(lib.srk_conv2d_backward_weight_grouped(ctypes.byref(d), n, xs, dys, masks, dws, dbs, 1.0, ptr(ws), ws.numel(),
                                                 stream_ptr()), "srk_conv2d_backward_weight_grouped")
    return ws   # (deferred reductions: the caller keeps the partial slabs alive until srk_wgrad_reduce_flush)


def flush_wgrads(on_group=None, max_layers=None):
    """Launch every recorded weight gradient (grouped by geometry).  `on_group(records)` runs after each group's
    launches — dp.DataParallel uses it to start that group's gradient bucket on its way."""
    if not _PENDING:
        return 0
    groups = pending_wgrad_groups(max_layers)
    del _PENDING[:]
    _DEFER["bytes"] = 0
    if on_group is not None or len(groups) < 2 or not MERGE_REDUCES:
        for recs in groups:
            launch_wgrad_group(recs)
            if on_group is not None:
                on_group(recs)
        return len(groups)
    # several launch groups and nobody waiting for one of them in particular: their slab reductions run as ONE launch
    # behind the last group (srk_wgrad_reduce_defer / _flush; the workspaces stay alive until then)
    lib = _lib.load()
    prev = lib.srk_wgrad_reduce_defer(1)
    keep = []   # the workspaces of the queued jobs: alive until the queue has run, on the error path as well
    try:
        for recs in groups:
            keep.append(launch_wgrad_group(recs))
        check(lib.srk_wgrad_reduce_flush(stream_ptr()), "srk_wgrad_reduce_flush")
    finally:
        lib.srk_wgrad_reduce_defer(prev)
        # a failure above may leave queued jobs behind: run them now (their slabs are still held by `keep`) rather than
        # inside somebody else's flush
        lib.srk_wgrad_reduce_flush(stream_ptr())
        del keep[:]
    return len(groups)


def drop_pending_wgrads():
    del _PENDING[:]
    _DEFER["bytes"] = 0


MERGE_REDUCES = True   # False: every weight-gradient launch group reduces its slabs itself
FUSE_SKIP_GRAD = True   # False: residual blocks sum their gradient fan-in with srk_axpby


class GradBox(object):
    """Gradient fan-in of a residual block without a separate add pass.  The block output gradient reaches the
    backward of the block's LAST conv as the gradient of its fused residual input; that backward parks it here
    (`res_box`) instead of returning it to autograd, and the backward of the block's FIRST conv -- which autograd
    runs later, and whose input is the same tensor as the skip -- hands it to srk_conv2d_backward_data as `add_to`
    (`add_box`), so dx = conv1^T(...) + dy_block comes out of the data-gradient kernel's epilogue."""
    __slots__ = ("g",)

    def __init__(self):
        self.g = None


class _Conv2d(torch.autograd.Function):
    """y = PS_r(act(conv(x, w) + b)) + residual, training-capable for act in {none, relu, lrelu}."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, cfg, packed, res_box=None, add_box=None):
        ctx.res_box, ctx.add_box = res_box, add_box
        require_cuda(x, weight, bias, residual)
        x = to_nhwc(x)
        if residual is not None:
            residual = to_nhwc(residual)
        ctx.wpb = None
        if packed is not None:
            wp, bp = packed[0], packed[1]
            if len(packed) > 2:
                ctx.wpb = packed[2]  # data-gradient layout already packed by the model's PackPlan
        else:
            wp = pack_weight_fwd(weight, cfg.transposed, cfg.ps_r)
            bp = pack_bias_ps(bias, cfg.ps_r)
        y = conv_forward_raw(x, wp, bp, weight, cfg, None, residual,
                             "train_fwd_tail" if (cfg.tail and LINEAR_TAIL_X3) else "train_fwd")
        ctx.cfg = cfg
        ctx.has_bias = bias is not None
        ctx.has_res = residual is not None
        ctx.weight_ref = weight
        ctx.bias_ref = bias
        need_mask = cfg.act in (ACT_RELU, ACT_LRELU)
        ctx.x_relu_out = _is_relu_output(x)      # x = relu(conv(..)): this conv's dx may leave pre-masked (see PREMASK)
        if cfg.act == ACT_RELU and residual is None and cfg.ps_r <= 1:
            y._srk_relu_out = _ver(y)
        ctx.save_for_backward(x, weight, y if need_mask else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        cfg = ctx.cfg
        x, weight, y = ctx.saved_tensors
        premasked = y is not None and cfg.act == ACT_RELU and _premasked_for(dy, y)
        PREMASK_STATS["masks_skipped"] += 1 if premasked else 0
        dy = to_nhwc(dy if (_is_nchw_dense(dy) or _is_nhwc_dense(dy)) else dy.contiguous())
        d = _make_desc(x.shape, weight, cfg, "bwd")
        dres = dy if ctx.has_res else None
        if ctx.has_res and ctx.res_box is not None:
            ctx.res_box.g, dres = dy, None  # consumed by the first conv of the block (GradBox)
        dyc = dy
        if cfg.ps_r > 1:
            r = cfg.ps_r
            # the bf16x3 data- and weight-gradient kernels read the pixel-shuffled dy directly (they un-shuffle while
            # staging their tiles); everything else gets an explicit depth-from-space pass first
            fused_ps = (d.algo in (ALGO_AUTO, _lib.ALGO_MFMA_BF16X3) and not cfg.transposed and cfg.stride == 1
                        and d.KH <= 3 and d.KW <= 3 and d.Cin >= 8 and (d.Cout // (r * r)) % 8 == 0)
            ctx_wpb = ctx.wpb
            if fused_ps:
                d.dy_ps_r = r
            else:
                ctx_wpb = None  # the PackPlan packs PS layers for the fused path ((i, j, c) contraction order)
                dyc = _empty_cl(d.N, d.Cout, d.OH, d.OW, dy)
                check(lib.srk_pixel_shuffle_backward(ptr(dy), ptr(dyc), d.N, d.OH, d.OW, d.Cout // (r * r), r,
                                                     stream_ptr()), "srk_pixel_shuffle_backward")
        mask = None
        if y is not None and not premasked:
            mask = BwdMask(ptr(y), cfg.slope if cfg.act == ACT_LRELU else 0.0)
        mref = ctypes.byref(mask) if mask is not None else None
        dx = dw = db = None
        need_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        wref, bref = ctx.weight_ref, (ctx.bias_ref if ctx.has_bias else None)
        wmask = (y if mask is not None else None, cfg.slope if cfg.act == ACT_LRELU else 0.0)
        flat_mode = _flat_grads(wref, bref) is not None
        if flat_mode:   # recorded for the grouped deferred launch, or launched here: before the data gradient
            _weight_grad(d, x, dyc, wref, bref, need_w, *wmask)
        if ctx.needs_input_grad[0]:
            plan_wpb = ctx.wpb if cfg.ps_r <= 1 else ctx_wpb
            wpb = plan_wpb if plan_wpb is not None else pack_weight_bwd(weight, cfg.transposed, d.dy_ps_r)
            dx = _empty_cl(d.N, d.Cin, d.H, d.W, dy)
            add_to = None
            if ctx.add_box is not None and ctx.add_box.g is not None:
                add_to, ctx.add_box.g = ctx.add_box.g, None
                if tuple(add_to.shape) != tuple(dx.shape):
                    raise RuntimeError("conv backward: skip gradient %s does not match dx %s"
                                       % (tuple(add_to.shape), tuple(dx.shape)))
            if (ctx.x_relu_out and _premask_on() and add_to is None and d.dy_ps_r <= 1 and not x.retains_grad
                    and lib.srk_conv2d_backward_data_relu_supported(ctypes.byref(d), ptr(dyc), ptr(dx), mref)):
                rc = lib.srk_conv2d_backward_data_relu(ctypes.byref(d), ptr(dyc), ptr(wpb), ptr(dx), mref, ptr(x),
                                                       stream_ptr())
                if rc == _lib.ERR_UNSUPPORTED:
                    # the applicability test passed but no tile of the wave-specialised kernel fits this problem: the
                    # standard data gradient, dx unmarked (the layer below applies its own mask) -- as the forward does
                    check(lib.srk_conv2d_backward_data(ctypes.byref(d), ptr(dyc), ptr(wpb), ptr(dx), mref, None,
                                                       stream_ptr()), "srk_conv2d_backward_data")
                else:
                    check(rc, "srk_conv2d_backward_data_relu")
                    dx._srk_premasked = (x.data_ptr(), _ver(dx))
                    PREMASK_STATS["masked_dx"] += 1
            else:
                check(lib.srk_conv2d_backward_data(ctypes.byref(d), ptr(dyc), ptr(wpb), ptr(dx), mref, ptr(add_to),
                                                   stream_ptr()), "srk_conv2d_backward_data")
        if not flat_mode:   # gradients autograd owns: after the data gradient
            dw, db = _weight_grad(d, x, dyc, wref, bref, need_w, *wmask)
        return dx, dw, db, dres, None, None, None, None


def conv2d(x, weight, bias=None, residual=None, cfg=None, packed=None, res_box=None, add_box=None):
    """Fused conv for training (act limited to none/relu/lrelu; no act together with residual/ps).
    res_box / add_box: see GradBox (both convs of a residual block share one box)."""
    cfg = cfg or ConvCfg()
    if cfg.act not in (ACT_NONE, ACT_RELU, ACT_LRELU):
        raise RuntimeError("conv2d (autograd path) fuses only none/relu/lrelu; use conv2d_infer or an unfused act")
    if cfg.act != ACT_NONE and (residual is not None or cfg.ps_r > 1):
        raise RuntimeError("conv2d (autograd path): activation cannot be fused together with residual/pixel-shuffle")
    return _Conv2d.apply(x, weight, bias, residual, cfg, packed, res_box, add_box)


LINEAR_TAIL_X3 = True


# ---- residual block with both convolutions in one launch (srk_resblock2_*) ----------------------------------------
RES2 = True   # False: residual blocks always run their two convs as separate launches


def _flat_grads(weight, bias):
    """(dw, db) views of the flat gradient buffer (optim.FlatParams) the kernels accumulate into, or None when autograd
    owns this layer's gradients."""
    wacc = getattr(weight, "_srk_grad", None)
    bacc = getattr(bias, "_srk_grad", None) if bias is not None else None
    return (wacc, bacc) if wacc is not None and (bias is None or bacc is not None) else None


def _weight_grad(d, x, dyc, weight, bias, need_w, mask_y=None, slope=0.0):
    """Weight / bias gradient of one conv -- the one place that records or launches one.  mask_y / slope: the output of
    a fused (leaky) ReLU whose mask the kernel applies to dyc.  Flat gradient buffers: recorded for the grouped deferred
    launch (flushed when the pass's records exceed DEFER_MAX_BYTES -- also under manual_wgrad_flush: those gradients are
    simply final before the exchange -- else by the engine callback the first record of a pass queues), or accumulated
    now (beta = 1).  Otherwise computed into fresh tensors.  Returns (dw, db) for autograd, (None, None) when
    accumulated in place."""
    if not need_w:
        return None, None
    lib = _lib.load()
    acc = _flat_grads(weight, bias)
    if acc is not None and DEFER_WGRAD:
        key = (d.N, d.H, d.W, d.Cin, d.OH, d.OW, d.Cout, d.KH, d.KW, d.stride, d.pad, d.transposed, d.out_pad,
               d.algo, d.dy_ps_r, acc[1] is not None, str(dyc.device))
        _PENDING.append(WgradRecord(key, d, x, dyc, mask_y, slope, *acc))
        _DEFER["bytes"] += 4 * (x.numel() + dyc.numel())
        if _DEFER["bytes"] > DEFER_MAX_BYTES:
            flush_wgrads()
        elif not _DEFER["queued"]:
            _DEFER["queued"] = True
            torch.autograd.Variable._execution_engine.queue_callback(_auto_flush)
        return None, None
    ws = torch.empty(max(int(lib.srk_conv2d_backward_weight_workspace_bytes(ctypes.byref(d))), 16), dtype=torch.uint8,
                     device=dyc.device)
    if acc is not None:
        dw, db, beta = acc + (1.0,)
    else:
        dw = torch.empty_like(weight, memory_format=torch.contiguous_format)
        db = torch.empty(d.Cout, dtype=torch.float32, device=dyc.device) if bias is not None else None
        beta = 0.0
    mask = ctypes.byref(BwdMask(ptr(mask_y), slope)) if mask_y is not None else None
    check(lib.srk_conv2d_backward_weight(ctypes.byref(d), ptr(x), ptr(dyc), mask, ptr(dw), ptr(db), beta, ptr(ws),
                                         ws.numel(), stream_ptr()), "srk_conv2d_backward_weight")
    return (None, None) if acc is not None else (dw, db)


def resblock2_applicable(x, w1, w2):
    """True when srk_resblock2_* can run this block: 3x3 C -> C -> C filters, a problem small enough that the fused
    tile pays (srk_resblock2_supported), and a precision mode whose kernels exist fused (not 'fp32')."""
    if not RES2 or x.dim() != 4 or os.environ.get("SRK_FORCE_ALGO"):
        return False
    n, c, h, w = x.shape
    if tuple(w1.shape) != (c, c, 3, 3) or tuple(w2.shape) != (c, c, 3, 3):
        return False
    mode = _MODES[_PRECISION["mode"]]
    if mode["train_fwd"] not in (ALGO_AUTO, _lib.ALGO_MFMA_BF16X3, _lib.ALGO_MFMA_BF16X6) or \
            mode["bwd"] not in (ALGO_AUTO, _lib.ALGO_MFMA_BF16X3, _lib.ALGO_MFMA_BF16X6):
        return False
    return bool(_lib.load().srk_resblock2_supported(n, h, w, c))


class _ResBlock2(torch.autograd.Function):
    """out = x + conv2(relu(conv1(x))) (base_networks.py:128-150, norm=None, activation='relu') as ONE forward and ONE
    data-gradient launch; the two weight gradients take the usual (grouped, deferred) path, without masks: the
    backward kernel hands out the already masked intermediate gradient."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, packed1, packed2):
        lib = _lib.load()
        require_cuda(x, w1, b1, w2, b2)
        x = to_nhwc(x)
        n, c, h, w = x.shape
        wp1 = packed1[0] if packed1 is not None else pack_weight_fwd(w1, False, 0)
        wp2 = packed2[0] if packed2 is not None else pack_weight_fwd(w2, False, 0)
        ctx.wpb1 = packed1[2] if packed1 is not None and len(packed1) > 2 else None
        ctx.wpb2 = packed2[2] if packed2 is not None and len(packed2) > 2 else None
        mid = _empty_cl(n, c, h, w, x)
        out = _empty_cl(n, c, h, w, x)
        algo = _MODES[_PRECISION["mode"]]["train_fwd"]
        xa = ya = None
        if F16X3:
            ya = _amax_alloc(x.device)
            if algo == _lib.ALGO_MFMA_BF16X6:   # fp32-faithful class: f16x3 (see F16X3 above)
                xa = amax_of(x, compute=F16X3_ALWAYS)
                if xa is not None:
                    algo = _lib.ALGO_MFMA_F16X3
        check(lib.srk_resblock2_forward(n, h, w, c, ptr(x), ptr(wp1), ptr(b1), ptr(wp2), ptr(b2), ptr(mid), ptr(out),
                                        algo, ptr(xa), ptr(ya), stream_ptr()), "srk_resblock2_forward")
        if ya is not None:
            _tag_amax(out, ya)
        ctx.refs = (w1, b1, w2, b2)
        ctx.save_for_backward(x, mid)
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, mid = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.refs
        n, c, h, w = x.shape
        dy = to_nhwc(dy if (_is_nchw_dense(dy) or _is_nhwc_dense(dy)) else dy.contiguous())
        wpb1 = ctx.wpb1 if ctx.wpb1 is not None else pack_weight_bwd(w1, False, 0)
        wpb2 = ctx.wpb2 if ctx.wpb2 is not None else pack_weight_bwd(w2, False, 0)
        dmid = _empty_cl(n, c, h, w, dy)
        dx = _empty_cl(n, c, h, w, dy)
        check(lib.srk_resblock2_backward_data(n, h, w, c, ptr(dy), ptr(wpb2), ptr(wpb1), ptr(mid), ptr(dmid), ptr(dx),
                                              _MODES[_PRECISION["mode"]]["bwd"], stream_ptr()),
              "srk_resblock2_backward_data")
        cfg = ConvCfg(1, 1, False, 0, ACT_NONE, 0.0, 0)
        d = _make_desc(x.shape, w1, cfg, "bwd")
        need = ctx.needs_input_grad
        # backward order of the separate convs: conv2 first (x = mid, dy = dy), then conv1 (x = x, dy = dmid)
        dw2, db2 = _weight_grad(_make_desc(x.shape, w2, cfg, "bwd"), mid, dy, w2, b2, need[3] or (b2 is not None and need[4]))
        dw1, db1 = _weight_grad(d, x, dmid, w1, b1, need[1] or (b1 is not None and need[2]))
        return (dx if need[0] else None), dw1, db1, dw2, db2, None, None


def resblock2(x, w1, b1, w2, b2, packed1=None, packed2=None):
    return _ResBlock2.apply(x, w1, b1, w2, b2, packed1, packed2)


def conv2d_infer(x, weight, bias=None, residual=None, cfg=None, prelu_w=None, packed=None):
    """No-grad fully fused conv: any activation + residual + pixel shuffle in one kernel."""
    cfg = cfg or ConvCfg()
    require_cuda(x, weight, bias, residual, prelu_w)
    cout, cin, _, _ = _weight_dims(weight, cfg.transposed)
    # the Cin <= 4 bf16x3 first-layer kernel reads the caller's NCHW tensor in place (no layout copy)
    # (also the f16x3 form of the fp32-faithful class; conv_forward_raw converts the layout if that kernel does not apply)
    x_nchw = (x.dim() == 4 and cin <= 4 and cout >= 8 and not cfg.transposed and not _is_nhwc_dense(x)
              and _is_nchw_dense(x)
              and (_algo_for(cfg, "infer") == ALGO_AUTO or (F16X3 and _algo_for(cfg, "infer") == _lib.ALGO_MFMA_BF16X6))
              and not os.environ.get("SRK_FORCE_ALGO"))  # (the debugging override may pick a kernel without the in-place NCHW read)
    if not x_nchw:
        x = to_nhwc(x)
    if residual is not None:
        residual = to_nhwc(residual)
    if packed is not None:
        wp, bp = packed
    else:
        wp = pack_weight_fwd(weight, cfg.transposed, cfg.ps_r)
        bp = pack_bias_ps(bias, cfg.ps_r)
    return conv_forward_raw(x, wp, bp, weight, cfg, prelu_w, residual, "infer", x_nchw)



# ---- ESPCN's first two convs in one launch (srk_espcn_pair_forward, conv_pair.hip) ------------------------------------
ESPCN_PAIR = True   # False: ESPCNNet.forward always runs its first two convs as separate launches
# An input without a maximum of its own is measured inside the fused launch up to this many bytes and by one srk_absmax
# pass in front of it above.  Inside the launch the maximum costs a chain of device-scope atomic round trips (about 8 us)
# plus the slice read at HBM speed, with nothing to hide behind; the pass costs 4 us plus its read on a busy queue, but a
# launch of its own where the host is the limit (34 against 37 us at 1.6 MB, the sizes between the library's
# efficiency rule and this threshold; 49 against 45 at 3 MB, 141 against 139 at 13 MB, 533 against 532 at c2's 50 MB).
PAIR_AMAX_IN_LAUNCH_BYTES = 2 << 20


def _pair_prepared(conv):
    """What srk_espcn_pair_prepare makes of the first layer's filter and bias, cached on the module the way its _PackCache
    keeps the packed filter: keyed by tensor and version."""
    from . import layers   # (layers imports this module)
    w, b = conv.weight, conv.bias
    key = (w.data_ptr(), _ver(w), b.data_ptr(), _ver(b), layers._WEIGHT_EPOCH[0], str(w.device))
    ent = getattr(conv, "_pair_prep", None)
    if ent is None or ent[0] != key:
        lib = _lib.load()
        buf = torch.empty((lib.srk_espcn_pair_prepared_bytes() + 3) // 4, dtype=torch.float32, device=w.device)
        check(lib.srk_espcn_pair_prepare(ptr(w.detach().contiguous()), ptr(b.detach().contiguous()), ptr(buf),
                                         stream_ptr()), "srk_espcn_pair_prepare")
        ent = conv._pair_prep = (key, buf)
    return ent[1]


def espcn_pair(x, block1, block2, force=False, scan=False):
    """relu(conv3x3(relu(conv5x5(x)))) of ESPCN's first two ConvBlocks as ONE launch (the 64-channel map between them
    stays on chip), or None where that kernel does not apply -- the caller then runs the blocks one by one.  Inference
    only, f16x3 arithmetic (the fp32-faithful class both layers run in on their own).  An x without a fresh maximum gets
    it inside the launch (no srk_absmax pass; up to PAIR_AMAX_IN_LAUNCH_BYTES) and is tagged with it afterwards.  force:
    skip the library's efficiency rule (tests).  scan: every block measures max|x| on the kernel's timeout path (tests)."""
    c1, c2 = block1.conv, block2.conv
    if not F16X3 or x.dim() != 4 or os.environ.get("SRK_FORCE_ALGO"):
        return None
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in (c1.weight, c1.bias, c2.weight, c2.bias)
                                                           if p is not None)):
        return None
    n, cin, h, w = x.shape
    if (cin != 3 or tuple(c1.weight.shape) != (64, 3, 5, 5) or tuple(c2.weight.shape) != (32, 64, 3, 3)
            or c1.bias is None or c2.bias is None or c1._s != 1 or c2._s != 1
            or c1._p != 0 or c2._p != 0 or h < 7 or w < 7):
        return None
    for b in (block1, block2):
        kind, _, _ = b._act_args()
        if kind != ACT_RELU or b.norm is not None:
            return None
    cfg1 = ConvCfg(c1._s, c1._p, False, 0, ACT_RELU, 0.0, 0)
    cfg2 = ConvCfg(c2._s, c2._p, False, 0, ACT_RELU, 0.0, 0)
    if _algo_for(cfg1, "infer") != _lib.ALGO_MFMA_BF16X6 or _algo_for(cfg2, "infer") != _lib.ALGO_MFMA_BF16X6:
        return None
    if not (x.dtype == torch.float32 and x.is_cuda and _is_nchw_dense(x)) or x.data_ptr() % 16:
        return None
    require_cuda(x, c1.weight, c1.bias, c2.weight, c2.bias)
    w1p = _pair_prepared(c1)
    b1 = c1.bias.detach().contiguous()
    wp2, bp2 = c2._cache.get(c2.weight, c2.bias, False, 0)
    a = getattr(x, "_srk_amax", None)   # a producer's maximum, a declared one, an earlier call's
    xa = a[0] if a is not None and a[1] == _ver(x) and a[2] == _AMAX_EPOCH[0] else None
    if xa is None and x.numel() * 4 > PAIR_AMAX_IN_LAUNCH_BYTES:
        xa = amax_of(x)
    measure = xa is None
    if measure:
        xa = _amax_alloc(x.device)   # zeroed: the kernel raises it
    y = _empty_cl(n, 32, h - 6, w - 6, x)
    ya = _amax_alloc(y.device)
    rc = _lib.load().srk_espcn_pair_forward(n, h, w, ptr(x), ptr(w1p), ptr(b1), ptr(wp2), ptr(bp2), ptr(y), ptr(xa),
                                            int(measure), ptr(ya), int(bool(force)) | (2 if scan else 0), stream_ptr())
    if rc == _lib.ERR_UNSUPPORTED:
        return None   # (nothing was launched: a buffer taken for the maximum is still zero and simply not used)
    check(rc, "srk_espcn_pair_forward")
    if measure:
        try:
            _tag_amax(x, xa)
        except Exception:  # noqa: BLE001 -- (a tensor subclass without a __dict__: measured again next time)
            pass
    _tag_amax(y, ya)
    return y


# ------------------------------------------------------------------------------------------------
# Pixel shuffle, activations, add / fork
# ------------------------------------------------------------------------------------------------
class _PixelShuffle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r):
        lib = _lib.load()
        require_cuda(x)
        x = to_nhwc(x)
        n, c, h, w = x.shape
        if c % (r * r):
            raise RuntimeError("pixel_shuffle: %d channels not divisible by r^2=%d" % (c, r * r))
        y = _empty_cl(n, c // (r * r), h * r, w * r, x)
        check(lib.srk_pixel_shuffle_forward(ptr(x), ptr(y), n, h, w, c // (r * r), r, stream_ptr()),
              "srk_pixel_shuffle_forward")
        ctx.r = r
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        r = ctx.r
        dy = to_nhwc(dy if (_is_nchw_dense(dy) or _is_nhwc_dense(dy)) else dy.contiguous())
        n, c, hr, wr = dy.shape
        dx = _empty_cl(n, c * r * r, hr // r, wr // r, dy)
        check(lib.srk_pixel_shuffle_backward(ptr(dy), ptr(dx), n, hr // r, wr // r, c, r, stream_ptr()),
              "srk_pixel_shuffle_backward")
        return dx, None


def pixel_shuffle(x, r):
    return _PixelShuffle.apply(x, int(r))


def _channels_inner(x):
    """Innermost (fastest) extent used for per-channel PReLU: C for NHWC 4-D, last dim for 2-D."""
    return x.shape[1] if x.dim() == 4 else x.shape[-1]


def _dense(x):
    """x in the layout the streaming kernels read (dense NHWC for 4-D, contiguous otherwise), starting on a 16-byte
    boundary: a dense view at an odd storage offset (`x[1:]` of a one-channel batch with H * W % 4 != 0) is copied --
    srk_act_forward / srk_axpby read float4 and refuse such a pointer."""
    if x.dim() == 4:
        x = to_nhwc(x if (_is_nchw_dense(x) or _is_nhwc_dense(x)) else x.contiguous())
    else:
        x = x.contiguous()
    if x.data_ptr() % 16:
        x = x.clone(memory_format=torch.preserve_format)
    return x


class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind, slope, prelu_w):
        lib = _lib.load()
        require_cuda(x, prelu_w)
        x = _dense(x)
        y = torch.empty_like(x)
        check(lib.srk_act_forward(ptr(x), ptr(y), x.numel(), _channels_inner(x), kind, slope, ptr(prelu_w),
                                  0 if prelu_w is None else prelu_w.numel(), stream_ptr()), "srk_act_forward")
        ctx.kind, ctx.slope = kind, slope
        ctx.prelu_ref = prelu_w
        ctx.save_for_backward(x if kind == ACT_PRELU else y, prelu_w)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        saved, prelu_w = ctx.saved_tensors
        dy = _dense(dy)
        dx = torch.empty_like(dy)
        dpw = ret_dpw = None
        if prelu_w is not None:
            dpw = getattr(ctx.prelu_ref, "_srk_grad", None)
            if dpw is None:
                dpw = ret_dpw = torch.zeros_like(prelu_w)
        check(lib.srk_act_backward(ptr(dy), ptr(saved), ptr(dx), dy.numel(), _channels_inner(dy), ctx.kind,
                                   ctx.slope, ptr(prelu_w), 0 if prelu_w is None else prelu_w.numel(), ptr(dpw),
                                   stream_ptr()), "srk_act_backward")
        return dx, None, None, ret_dpw


def activation(x, kind, slope=0.0, prelu_w=None):
    if isinstance(kind, str) or kind is None:
        kind = ACT_BY_NAME[kind]
    if kind == ACT_NONE:
        return x
    if kind == ACT_LRELU and float(slope) < 0.0:
        # the backward decides the side by the sign of the saved OUTPUT, which a negative slope flips
        raise RuntimeError("activation: LeakyReLU with a negative slope (%g) is not supported" % float(slope))
    return _Act.apply(x, int(kind), float(slope), prelu_w)


def _axpby(a, b, alpha, beta):
    lib = _lib.load()
    out = torch.empty_like(a)
    check(lib.srk_axpby(ptr(a), ptr(b), ptr(out), a.numel(), alpha, beta, stream_ptr()), "srk_axpby")
    return out


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        require_cuda(a, b)
        if a.shape != b.shape:
            raise RuntimeError("add: shape mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        a, b = _dense(a), _dense(b)
        return _axpby(a, b, 1.0, 1.0)

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    """torch.add(out, residual) of the reference (base_networks.py:149, vdsr.py:31, edsr.py:42)."""
    return _Add.apply(a, b)


class _Axpby(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, alpha, beta):
        require_cuda(a, b)
        if b is not None and a.shape != b.shape:
            raise RuntimeError("axpby: shape mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        ctx.ab = (alpha, beta)
        a = _dense(a)
        return _axpby(a, a if b is None else _dense(b), alpha, beta if b is not None else 0.0)

    @staticmethod
    def backward(ctx, g):
        alpha, beta = ctx.ab
        g = _dense(g)
        return (_axpby(g, g, alpha, 0.0) if ctx.needs_input_grad[0] else None,
                _axpby(g, g, beta, 0.0) if ctx.needs_input_grad[1] else None, None, None)


def axpby(a, b, alpha, beta=0.0):
    """alpha * a + beta * b (b None: alpha * a) on srk_axpby, each gradient one srk_axpby launch: VESPCN's flow in
    pixels, max_flow * coarse + max_flow / 4 * fine."""
    return _Axpby.apply(a, b, float(alpha), float(beta))


class _Fork(torch.autograd.Function):
    """Use a tensor twice (trunk + skip) with the gradient fan-in summed by srk_axpby instead of
    autograd's internal ATen add."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, g1, g2):
        if g1 is None:
            return g2
        if g2 is None:
            return g1
        return _axpby(_dense(g1), _dense(g2), 1.0, 1.0)


def fork(x):
    a, b = _Fork.apply(x)
    t = getattr(x, "_srk_amax", None)      # the views carry the running maximum of the tensor they alias
    if t is not None and t[1] == _ver(x) and t[2] == _AMAX_EPOCH[0]:
        _tag_amax(a, t[0])
        _tag_amax(b, t[0])
    return a, b


# ------------------------------------------------------------------------------------------------
# Losses (mean reduction), forward + gradient in one pass
# ------------------------------------------------------------------------------------------------
# Seeds of a backward pass.  `loss.backward()` makes autograd fill a ones tensor (one ATen launch) and the loss backward
# multiply its stored gradient by it (srk_scale_dev, a second launch); a data-parallel step seeds with 1/world instead.
# The train steps of this package know their seed when they compute the loss:
#   * backward(loss) seeds with a persistent per-device ones tensor, which the loss backward recognises (by address) and
#     answers with the gradient the forward already wrote -- no fill, no scale;
#   * inside `with loss_seed(value, tensor):` the loss forward folds `value` into that gradient, and a backward seeded with
#     `tensor` (dp.loss_seed) skips the multiply as well.
# Any other upstream gradient (a weighted sum of losses, user code) takes the general path.
# This is the seed contract of every scalar loss here (the pixel, SSIM and FFT losses, drcn_head, lpips, ragan_loss,
# gan_logit_loss), and three functions hold it: _declare_seed in the forward, _is_own_seed and _seed_scaled in the backward.
_UNIT = {}
_LOSS_SEED = [None]


def _device_index(device):
    return device.index if device.index is not None else torch.cuda.current_device()


def unit_seed(device):
    idx = _device_index(device)
    t = _UNIT.get(idx)
    if t is None:
        t = _UNIT[idx] = torch.ones((), dtype=torch.float32, device=torch.device("cuda", idx))
    return t


def backward(losses, seed=None):
    """torch.autograd.backward(losses) seeded with the persistent ones tensor of the device (or `seed` for each loss)."""
    losses = list(losses) if isinstance(losses, (list, tuple)) else [losses]
    g = unit_seed(losses[0].device) if seed is None else seed
    torch.autograd.backward(losses, [g] * len(losses))


class loss_seed(object):
    """Context: losses computed inside store their gradient already multiplied by `value`; a backward pass seeded with
    `tensor` (which must hold `value`) then uses it as is.  The seed is recognised by its address; every loss node
    computed inside keeps `tensor` alive until its graph is freed, so no other gradient can come to live at that address."""

    def __init__(self, value, tensor):
        self.seed = (float(value), tensor)

    def __enter__(self):
        self.prev, _LOSS_SEED[0] = _LOSS_SEED[0], self.seed

    def __exit__(self, *a):
        _LOSS_SEED[0] = self.prev


def _declare_seed(ctx, declare=True):
    """Forward of a loss node: records the seed declared by loss_seed (none where `declare` is false) on the ctx and
    returns the value the kernel folds into the gradient it stores, 1.0 when none is declared."""
    seed = _LOSS_SEED[0] if declare else None
    ctx.seed_ptr, ctx.seed_value = (seed[1].data_ptr(), seed[0]) if seed is not None else (0, 1.0)
    # the declared seed is recognised by its address, so the node keeps the tensor alive: freed, its block could
    # be handed to another upstream gradient, which would then pass for the declared one
    ctx.seed_keep = seed[1] if seed is not None else None
    return ctx.seed_value


def _is_own_seed(ctx, g, device):
    """Backward of a loss node: whether the upstream gradient g is the seed the stored gradient was computed for -- the
    declared seed or, with none declared, the unit seed of the device (under a declared seed the unit seed is as foreign
    as any other gradient).  A foreign g is a factor on the stored gradient, after g / ctx.seed_value has undone a
    folded seed: _seed_scaled applies it in fp32, _LpipsFinish to its fp64 row."""
    return g.data_ptr() == (ctx.seed_ptr if ctx.seed_ptr else unit_seed(device).data_ptr())


def _seed_scaled(ctx, g, grads):
    """The stored fp32 gradients `grads` (a tuple, None where an operand takes none) as the backward hands them out: as
    they are under the node's own seed, else each times the foreign g (srk_scale_dev into a fresh tensor, one launch per
    gradient).  They stay on the ctx, not in save_for_backward: a second backward over a retained graph sees them, and
    they are freed with the graph."""
    live = [d for d in grads if d is not None]
    if not live or _is_own_seed(ctx, g, live[0].device):
        return grads
    lib = _lib.load()
    g = (g / ctx.seed_value if ctx.seed_ptr else g).contiguous()
    outs = tuple(None if d is None else torch.empty_like(d) for d in grads)
    for d, out in zip(grads, outs):
        if d is not None:
            check(lib.srk_scale_dev(ptr(d), ptr(g), ptr(out), d.numel(), stream_ptr()), "srk_scale_dev")
    return outs


def _loss_inputs(ctx, pred, target, ws_bytes):
    """What the pixel, SSIM and FFT losses do before their launch: pred dense as [N,C,H,W] (or [B, F] as N = B, C = F,
    H = W = 1: BCE on the discriminator output), the target's strides, and the loss, gradient (None where pred takes
    none) and workspace (ws_bytes(n, c, h, w) bytes) to write."""
    require_cuda(pred, target)
    if pred.shape != target.shape:
        raise RuntimeError("loss: pred %s vs target %s" % (tuple(pred.shape), tuple(target.shape)))
    if pred.dim() == 4:
        pred = _dense(pred)
        n, c, h, w = pred.shape
        ts = target.stride()
    else:
        pred = pred.contiguous()
        n, c = pred.shape[0], pred.numel() // pred.shape[0]
        h = w = 1
        target = target.contiguous()
        ts = (c, 1, 1, 1)
    strides = (ctypes.c_int64 * 4)(*[int(s) for s in ts])
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
    ws = torch.empty(int(ws_bytes(n, c, h, w)), dtype=torch.uint8, device=pred.device)
    return pred, target, strides, (n, c, h, w), loss, dpred, ws


class _PixelLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, kind, eps):
        lib = _lib.load()
        ws_bytes = lambda *dims: lib.srk_loss_workspace_bytes()
        pred, target, strides, dims, loss, dpred, ws = _loss_inputs(ctx, pred, target, ws_bytes)
        check(lib.srk_loss_forward_backward(kind, ptr(pred), ptr(target), strides, *dims, eps, _declare_seed(ctx),
                                            ptr(loss), ptr(dpred), ptr(ws), stream_ptr()), "srk_loss_forward_backward")
        ctx.grads = (dpred,)
        return loss

    @staticmethod
    def backward(ctx, g):
        return _seed_scaled(ctx, g, ctx.grads) + (None, None, None)


class _SSIMLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        lib = _lib.load()
        if pred.dim() != 4 or min(pred.shape[2:]) < 11:
            raise RuntimeError("ssim_loss: takes [N,C,H,W] with planes of at least the 11 x 11 window, got shape %s"
                               % (tuple(pred.shape),))
        ws_bytes = lambda *dims: lib.srk_ssim_loss_workspace_bytes()
        pred, target, strides, dims, loss, dpred, ws = _loss_inputs(ctx, pred, target, ws_bytes)
        check(lib.srk_ssim_loss_forward_backward(ptr(pred), ptr(target), strides, *dims, _declare_seed(ctx), ptr(loss),
                                                 ptr(dpred), ptr(ws), stream_ptr()), "srk_ssim_loss_forward_backward")
        ctx.grads = (dpred,)
        return loss

    @staticmethod
    def backward(ctx, g):
        return _seed_scaled(ctx, g, ctx.grads) + (None,)


class _FFTLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, ortho):
        lib = _lib.load()
        if pred.dim() != 4 or min(pred.shape) < 1:
            raise RuntimeError("fft_loss: takes non-empty [N,C,H,W], got shape %s" % (tuple(pred.shape),))
        if max(pred.shape[2:]) > _lib.FFT_LOSS_MAX_DIM:
            raise RuntimeError("fft_loss: planes of %d x %d, the dense DFT takes at most %d on a side"
                               % (pred.shape[2], pred.shape[3], _lib.FFT_LOSS_MAX_DIM))
        pred, target, strides, dims, loss, dpred, ws = _loss_inputs(ctx, pred, target, lib.srk_fft_loss_workspace_bytes)
        h, w = dims[2:]
        scale = 1.0 / math.sqrt(float(h) * float(w)) if ortho else 1.0
        tables = _dft_tables(h, w, pred.device)
        check(lib.srk_fft_loss_forward_backward(ptr(pred), ptr(target), strides, *dims, ptr(tables), scale,
                                                _declare_seed(ctx), ptr(loss), ptr(dpred), ptr(ws), stream_ptr()),
              "srk_fft_loss_forward_backward")
        ctx.grads = (dpred,)
        return loss

    @staticmethod
    def backward(ctx, g):
        return _seed_scaled(ctx, g, ctx.grads) + (None, None)


_CONSTS = {}


def _const_scalar(value, device):
    """A persistent 0-dim device tensor holding `value` (loss weights, label rows): no fill launch per step."""
    idx = _device_index(device)
    key = (float(value), idx)
    t = _CONSTS.get(key)
    if t is None:
        t = _CONSTS[key] = torch.full((), float(value), dtype=torch.float32, device=torch.device("cuda", idx))
    return t


def const_rows(value, rows, device):
    """Persistent [rows, 1] label tensor (torch.ones(B, 1) / zeros(B, 1) of srgan.py:264-265 without a fill per step)."""
    idx = _device_index(device)
    key = (float(value), int(rows), idx)
    t = _CONSTS.get(key)
    if t is None:
        t = _CONSTS[key] = torch.full((int(rows), 1), float(value), dtype=torch.float32, device=torch.device("cuda", idx))
    return t


class _LossSum(torch.autograd.Function):
    """a * l1 + b * l2 of two scalar losses with srk_axpby (D_loss = real + fake, G_loss = mse + 1e-3 * GAN:
    srgan.py:283,306); seeded by the unit seed, the backward hands out persistent constants -- no ATen arithmetic in
    the captured step."""

    @staticmethod
    def forward(ctx, l1, l2, a, b):
        ctx.ab = (float(a), float(b))
        return _axpby(l1.reshape(1), l2.reshape(1), float(a), float(b)).reshape(())

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.ab
        if g.data_ptr() == unit_seed(g.device).data_ptr():
            return (g if a == 1.0 else _const_scalar(a, g.device)), (g if b == 1.0 else _const_scalar(b, g.device)), None, None
        return (g if a == 1.0 else g * a), (g if b == 1.0 else g * b), None, None


def loss_sum(l1, l2, a=1.0, b=1.0):
    return _LossSum.apply(l1, l2, a, b)


def weighted_term(loss_fn, weight, pred, target):
    """loss_fn(pred, target) as a term that loss_sum will weigh by `weight`.  Where no seed is declared yet (one GPU) the
    weight is declared as the term's seed, with the very constant that _LossSum.backward hands out under the unit seed:
    the loss kernel folds it into its gradient and the backward returns that as it is, instead of a srk_scale_dev pass
    over the whole gradient per term.  Under a declared seed (data parallel), or for a weight of 0 or 1 (which
    _LossSum answers with its own upstream gradient), the term is computed plainly and takes the general path."""
    if _LOSS_SEED[0] is None and 0.0 < weight < 1.0:
        with loss_seed(weight, _const_scalar(weight, pred.device)):
            return loss_fn(pred, target)
    return loss_fn(pred, target)


def mse_loss(pred, target):
    """nn.MSELoss() (srcnn.py:84-86,129; vdsr.py:145; srgan.py:205,300)."""
    return _PixelLoss.apply(pred, target, _lib.LOSS_MSE, 0.0)


def l1_loss(pred, target):
    """nn.L1Loss() (edsr.py:98-100,153)."""
    return _PixelLoss.apply(pred, target, _lib.LOSS_L1, 0.0)


def charbonnier_loss(pred, target, eps=1e-6):
    """L1_Charbonnier_loss (lapsrn.py:75-85)."""
    return _PixelLoss.apply(pred, target, _lib.LOSS_CHARBONNIER, float(eps))


def bce_loss(pred, target):
    """nn.BCELoss() (srgan.py:157,276-297)."""
    return _PixelLoss.apply(pred, target, _lib.LOSS_BCE, 0.0)


def ssim_loss(pred, target):
    """1 - mean SSIM of pred against target (11 x 11 Gaussian window, valid positions, L = 1, every plane and position
    weighing the same; pred is read UNCLAMPED so that out-of-range pixels keep their gradient): the loss and its
    gradient from one launch, under the seed contract of the losses (_declare_seed).
    [N,C,H,W] with H, W >= 11.  include/srk.h: srk_ssim_loss_forward_backward."""
    return _SSIMLoss.apply(pred, target)


_DFT_TABLES = {}
FFT_NORMS = ("backward", "ortho")


def _dft_tables(h, w, device):
    """The twiddle tables of srk_dft_table_host for H then W as one fp64 device tensor, uploaded once per (H, W, device):
    the device computes no cos / sin of its own.  The first use of a size must come before a graph capture (a warm-up
    step does it): the upload is a host-to-device copy."""
    idx = _device_index(device)
    key = (int(h), int(w), idx)
    t = _DFT_TABLES.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("fft_loss: the twiddle tables of %d x %d are not on the device yet; run one step before "
                               "capturing" % (h, w))
        lib = _lib.load()
        host = torch.empty(2 * (int(h) + int(w)), dtype=torch.float64)
        base = ctypes.cast(host.data_ptr(), ctypes.POINTER(ctypes.c_double))
        check(lib.srk_dft_table_host(int(h), base), "srk_dft_table_host")
        check(lib.srk_dft_table_host(int(w), ctypes.cast(host.data_ptr() + 16 * int(h), ctypes.POINTER(ctypes.c_double))),
              "srk_dft_table_host")
        t = _DFT_TABLES[key] = host.to(torch.device("cuda", idx))
    return t


def fft_loss(pred, target, norm="backward"):
    """The frequency-domain loss of BasicSR's FFTLoss, nn.L1Loss()(view_as_real(fft2(pred)), view_as_real(fft2(target)))
    with fft2's `norm` ("backward": unscaled, "ortho": 1 / sqrt(H W)), over the full spectrum of every plane: a dense
    fp64 DFT on tables from the host, so the bits do not depend on a library's plan and Im F is an exact zero at the
    self-conjugate bins.  Loss and gradient from one call, under the seed contract of the losses
    (_declare_seed).  [N,C,H,W] with H, W <= 256.  include/srk.h: srk_fft_loss_forward_backward."""
    if norm not in FFT_NORMS:
        raise ValueError("fft_loss: norm %r is not one of %s" % (norm, FFT_NORMS))
    return _FFTLoss.apply(pred, target, norm == "ortho")


# ------------------------------------------------------------------------------------------------
# BatchNorm2d / Linear (SRGAN)
# ------------------------------------------------------------------------------------------------
BN_FIN_APPLY = True   # False: split reductions as launches of their own (rounds 1 - 5)


# Collectives inside a captured step (SyncBN's [2C] sums): a capture cannot hold them, so the capturing side
# (trainers.GraphedSegments with a _Splitter) cuts its graph there -- end the graph, run the collective eagerly now and at
# every replay, begin the next graph.  Outside a capture the collective simply runs.
_SPLITTER = [None]


def _collective(fn):
    sp = _SPLITTER[0]
    if sp is not None and torch.cuda.is_current_stream_capturing():
        sp.collective(fn)
    else:
        fn()


def _bn_train_stats(lib, x, rows, c, mean, rstd, stats, running, momentum, eps, nbt_p, sync_group, fin):
    """The four ways to a training BatchNorm's statistics.  Returns (count, partials): with `fin` (finalize-in-apply) the
    column sums are left as partials = (tensor, splits) for srk_bn_finalize_apply_act; otherwise mean / rstd / the running
    statistics are written here and partials is None."""
    ws = torch.empty(int(lib.srk_bn_workspace_bytes(c)), dtype=torch.uint8, device=x.device)
    part = getattr(x, "_srk_bn_partial", None)   # column sums from the producing conv's epilogue (k_c64)
    if part is not None and (sync_group is not None or part[2] != _ver(x) or part[0].shape[1] != 2 * c):
        part = None
    rm, rv = running
    if fin:
        if part is not None:
            return float(rows), (part[0], int(part[1]))
        sp = ctypes.c_int(0)
        check(lib.srk_bn_stats_partials(ptr(x), rows, c, ptr(ws), ctypes.byref(sp), stream_ptr()), "srk_bn_stats_partials")
        return float(rows), (ws, int(sp.value))
    if part is not None:             # reduce + finalize only
        check(lib.srk_bn_finalize_partials(ptr(part[0]), part[1], ptr(stats), rows, c, ptr(mean), ptr(rstd), ptr(rm), ptr(rv),
                                           momentum, eps, nbt_p, stream_ptr()), "srk_bn_finalize_partials")
        return float(rows), None
    if sync_group is None:           # column sums, then reduce + mean / rstd / running statistics
        check(lib.srk_bn_stats_finalize(ptr(x), ptr(stats), rows, c, ptr(mean), ptr(rstd), ptr(rm), ptr(rv), momentum, eps,
                                        nbt_p, ptr(ws), stream_ptr()), "srk_bn_stats_finalize")
        return float(rows), None
    import torch.distributed as dist   # SyncBN: the [2C] sums are all-reduced between the two phases
    check(lib.srk_bn_stats(ptr(x), ptr(stats), rows, c, ptr(ws), stream_ptr()), "srk_bn_stats")
    _collective(lambda: dist.all_reduce(stats, group=sync_group))
    count = float(rows) * dist.get_world_size(sync_group)
    check(lib.srk_bn_finalize(ptr(stats), count, ptr(mean), ptr(rstd), ptr(rm), ptr(rv), momentum, eps, c, nbt_p,
                              stream_ptr()), "srk_bn_finalize")
    return count, None


class _BatchNorm(torch.autograd.Function):
    """y = act(bn(x)) [+ residual].  act in {none, relu, lrelu, prelu} and the residual ride in the BatchNorm kernels
    (srk_bn_*_act): the backward recomputes z = gamma * xhat + beta from x, so nothing of the activation is saved."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, sync_group, nbt=None,
                act=ACT_NONE, slope=0.0, prelu_w=None, residual=None, res_box=None):
        lib = _lib.load()
        ctx.res_box = res_box
        require_cuda(x, gamma, beta, prelu_w, residual)
        x = _dense(x)   # [N,C,H,W] stored NHWC, or [B,F] (BatchNorm1d of DenseBlock, base_networks.py:13): rows x C
        c = x.shape[1]
        rows = x.numel() // c
        mean = torch.empty(c, dtype=torch.float32, device=x.device)
        rstd = torch.empty(c, dtype=torch.float32, device=x.device)
        aligned = all(t is None or t.data_ptr() % 16 == 0 for t in (x, gamma, beta, residual))
        pn = 0 if prelu_w is None else prelu_w.numel()
        count, part = float(rows), None
        if training:
            stats = torch.empty(2 * c, dtype=torch.float64, device=x.device)
            if nbt is not None and (nbt.dtype != torch.int64 or not nbt.is_cuda):
                raise RuntimeError("batch_norm: num_batches_tracked must be a CUDA int64 tensor")
            nbt_p = None if nbt is None else ctypes.c_void_p(nbt.data_ptr())
            # finalize-in-apply (round 6): the apply kernel finishes the split reduction itself -- one launch less
            fin = bool(BN_FIN_APPLY and sync_group is None and lib.srk_bn_fused_supported(c) and aligned)
            count, part = _bn_train_stats(lib, x, rows, c, mean, rstd, stats, (running_mean, running_var), momentum, eps,
                                          nbt_p, sync_group, fin)
        else:
            check(lib.srk_bn_eval_params(ptr(running_mean), ptr(running_var), eps, ptr(mean), ptr(rstd), c,
                                         stream_ptr()), "srk_bn_eval_params")
        y = torch.empty_like(x)
        # 4-D activations in front of a convolution of the fp32-faithful class: leave the output's running maximum
        # (only on the kernels' 16-byte path -- C % 4 == 0, aligned tensors; an unaligned view takes the scalar kernel,
        # which keeps no maximum: the convolution behind it then stays on the six-MFMA arithmetic)
        ya = _amax_alloc(x.device) if (F16X3 and x.dim() == 4 and c % 4 == 0 and aligned
                                       and (F16X3_ALWAYS or rows * ((c + 63) // 64) >= F16X3_MIN_PIXELS)
                                       and _MODES[_PRECISION["mode"]]["train_fwd" if training else "infer"]
                                       in (_lib.ALGO_MFMA_BF16X6, _lib.ALGO_MFMA_F16X3)) else None
        if residual is not None:
            residual = _dense(residual)
            if tuple(residual.shape) != tuple(x.shape) or residual.stride() != x.stride():
                raise RuntimeError("batch_norm: residual must have the shape and layout of x")
        if part is not None:
            check(lib.srk_bn_finalize_apply_act(ptr(part[0]), part[1], ptr(stats), rows, c, ptr(mean), ptr(rstd),
                                                ptr(running_mean), ptr(running_var), momentum, eps, nbt_p, ptr(x), ptr(y),
                                                ptr(gamma), ptr(beta), act, slope, ptr(prelu_w), pn, ptr(residual), ptr(ya),
                                                stream_ptr()), "srk_bn_finalize_apply_act")
        elif act != ACT_NONE or residual is not None:
            check(lib.srk_bn_apply_act(ptr(x), ptr(y), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), rows, c, act, slope,
                                       ptr(prelu_w), pn, ptr(residual), ptr(ya), stream_ptr()), "srk_bn_apply_act")
        else:   # (the plain kernels round the affine differently from the _act ones: kept)
            check(lib.srk_bn_apply(ptr(x), ptr(y), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), rows, c, ACT_NONE, 0.0,
                                   ptr(ya), stream_ptr()), "srk_bn_apply")
        if ya is not None:
            _tag_amax(y, ya)    # the convolution behind a BatchNorm scales its fp16 planes by this (F16X3)
        ctx.training, ctx.count, ctx.sync_group = training, count, sync_group
        ctx.fin = part is not None
        ctx.gamma_ref, ctx.beta_ref, ctx.prelu_ref = gamma, beta, prelu_w
        ctx.act, ctx.slope, ctx.has_res = act, slope, residual is not None
        ctx.save_for_backward(x, gamma, mean, rstd, beta if act != ACT_NONE else None, prelu_w)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, gamma, mean, rstd, beta, prelu_w = ctx.saved_tensors
        dy = _dense(dy)
        c = x.shape[1]
        rows = x.numel() // c
        dstats = torch.empty(2 * c, dtype=torch.float64, device=x.device)
        ws = torch.empty(int(lib.srk_bn_workspace_bytes(c)), dtype=torch.uint8, device=x.device)
        dgamma = getattr(ctx.gamma_ref, "_srk_grad", None)
        dbeta = getattr(ctx.beta_ref, "_srk_grad", None)
        ret_g = ret_b = ret_p = dprelu = None
        if dgamma is None or dbeta is None:
            dgamma = ret_g = torch.zeros(c, dtype=torch.float32, device=x.device)
            dbeta = ret_b = torch.zeros(c, dtype=torch.float32, device=x.device)
        pn = 0 if prelu_w is None else prelu_w.numel()
        if ctx.act == ACT_PRELU:
            dprelu = getattr(ctx.prelu_ref, "_srk_grad", None)
            if dprelu is None:
                dprelu = ret_p = torch.zeros_like(prelu_w)
        dres = dy if ctx.has_res else None   # the residual's gradient is dy itself
        if ctx.has_res and ctx.res_box is not None:
            ctx.res_box.g, dres = dy, None   # parked for the block's first conv, which adds it in its data-gradient kernel
        dx = torch.empty_like(dy)
        act_args = (ctx.act, ctx.slope, ptr(prelu_w), pn)
        if ctx.fin and dy.data_ptr() % 16 == 0:
            # finalize-in-apply: column sums, then ONE kernel that reduces them (per 16-channel slab), adds the parameter
            # gradients and writes dx
            sp = ctypes.c_int(0)
            check(lib.srk_bn_backward_partials_act(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), rows, c,
                                                   *act_args, ptr(ws), ctypes.byref(sp), stream_ptr()),
                  "srk_bn_backward_partials_act")
            check(lib.srk_bn_backward_finalize_apply_act(ptr(ws), int(sp.value), ptr(dstats), ctx.count, ptr(dy), ptr(x),
                                                         ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(dx), rows, c,
                                                         ptr(dgamma), ptr(dbeta), *act_args, ptr(dprelu), stream_ptr()),
                  "srk_bn_backward_finalize_apply_act")
        else:
            # statistics of the backward + the parameter gradients (from the LOCAL sums: the DP gradient all-reduce happens
            # later), then dx; SyncBN all-reduces the sums in between
            check(lib.srk_bn_backward_stats_grads_act(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
                                                      ptr(dstats), rows, c, ptr(dgamma), ptr(dbeta), *act_args, ptr(dprelu),
                                                      ptr(ws), stream_ptr()), "srk_bn_backward_stats_grads_act")
            if ctx.training and ctx.sync_group is not None:
                import torch.distributed as dist
                grp = ctx.sync_group
                _collective(lambda: dist.all_reduce(dstats, group=grp))
            if not ctx.training:   # eval-mode BN: statistics are constants -> no mean / projection terms in dx
                dstats = torch.zeros_like(dstats)
            check(lib.srk_bn_backward_apply_act(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(dstats),
                                                ctx.count, ptr(dx), rows, c, *act_args, stream_ptr()),
                  "srk_bn_backward_apply_act")
        return dx, ret_g, ret_b, None, None, None, None, None, None, None, None, None, ret_p, dres, None


def batch_norm(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5, sync_group=None,
               num_batches_tracked=None, act=ACT_NONE, slope=0.0, prelu_w=None, residual=None, res_box=None):
    """nn.BatchNorm2d (base_networks.py:46,117,161) on [N,C,H,W]; nn.BatchNorm1d (base_networks.py:13) on [B,F].
    act / prelu_w / residual: y = act(bn(x)) [+ residual] in the same launches (see bn_fusable).  res_box: GradBox the
    residual's gradient is parked in instead of being returned to autograd (the block's first conv adds it)."""
    return _BatchNorm.apply(x, gamma, beta, running_mean, running_var, bool(training), float(momentum), float(eps),
                            sync_group, num_batches_tracked, int(act), float(slope), prelu_w, residual, res_box)


def bn_fusable(x, act, prelu_w=None, bn=None):
    """Can `act` (and a residual add) ride in the BatchNorm kernels for this input?  ReLU / LeakyReLU / PReLU with one
    slope or one per channel, channel count a multiple of 4 (the fused kernels move float4s), per-shard statistics
    (SyncBN keeps the separate passes)."""
    if bn is not None and getattr(bn, "sync_group", None) is not None:
        return False
    if act not in (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_PRELU) or x.dim() < 2 or x.shape[1] % 4:
        return False
    return act != ACT_PRELU or (prelu_w is not None and prelu_w.numel() in (1, x.shape[1]))


class _InstanceNorm(torch.autograd.Function):
    """nn.InstanceNorm2d defaults (affine=False, no running statistics; base_networks.py:48,83,119,163): every
    (sample, channel) plane is normalised with its own biased statistics.  A sample of an NHWC tensor is a dense
    [H*W, C] matrix, so this is the BatchNorm kernels applied per sample (unused by every reference net: N small
    launches rather than a dedicated kernel)."""

    @staticmethod
    def forward(ctx, x, eps):
        lib = _lib.load()
        require_cuda(x)
        x = _dense(x)
        n, c, h, w = x.shape
        rows = h * w
        mean = torch.empty((n, c), dtype=torch.float32, device=x.device)
        rstd = torch.empty((n, c), dtype=torch.float32, device=x.device)
        stats = torch.empty(2 * c, dtype=torch.float64, device=x.device)
        ws = torch.empty(int(lib.srk_bn_workspace_bytes(c)), dtype=torch.uint8, device=x.device)
        y = torch.empty_like(x)
        xs, ys = x.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1)   # [n][h][w][c] views of the NHWC storage
        for i in range(n):
            check(lib.srk_bn_stats(ptr(xs[i]), ptr(stats), rows, c, ptr(ws), stream_ptr()), "srk_bn_stats")
            check(lib.srk_bn_finalize(ptr(stats), float(rows), ptr(mean[i]), ptr(rstd[i]), None, None, 0.0, eps, c, None,
                                      stream_ptr()), "srk_bn_finalize")
            check(lib.srk_bn_apply(ptr(xs[i]), ptr(ys[i]), ptr(mean[i]), ptr(rstd[i]), None, None, rows, c, ACT_NONE, 0.0,
                                   None, stream_ptr()), "srk_bn_apply")
        ctx.save_for_backward(x, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, mean, rstd = ctx.saved_tensors
        dy = _dense(dy)
        n, c, h, w = x.shape
        rows = h * w
        dstats = torch.empty(2 * c, dtype=torch.float64, device=x.device)
        ws = torch.empty(int(lib.srk_bn_workspace_bytes(c)), dtype=torch.uint8, device=x.device)
        dx = torch.empty_like(dy)
        xs, dys, dxs = x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1)
        for i in range(n):
            check(lib.srk_bn_backward_stats(ptr(dys[i]), ptr(xs[i]), ptr(mean[i]), ptr(rstd[i]), ptr(dstats), rows, c,
                                            ptr(ws), stream_ptr()), "srk_bn_backward_stats")
            check(lib.srk_bn_backward_apply(ptr(dys[i]), ptr(xs[i]), ptr(mean[i]), ptr(rstd[i]), None, ptr(dstats),
                                            float(rows), ptr(dxs[i]), rows, c, stream_ptr()), "srk_bn_backward_apply")
        return dx, None


def instance_norm(x, eps=1e-5):
    """nn.InstanceNorm2d(C) with its defaults (base_networks.py:48)."""
    return _InstanceNorm.apply(x, float(eps))


class _RowNorm(torch.autograd.Function):
    """nn.InstanceNorm1d on a [B, F] activation (DenseBlock(norm='instance'), base_networks.py:12-13): every row normalised
    with its own biased statistics (srk_rownorm_*)."""

    @staticmethod
    def forward(ctx, x, eps):
        lib = _lib.load()
        require_cuda(x)
        x = x.contiguous()
        rows, cols = x.shape
        y = torch.empty_like(x)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        check(lib.srk_rownorm_forward(ptr(x), ptr(y), ptr(mean), ptr(rstd), rows, cols, eps, stream_ptr()),
              "srk_rownorm_forward")
        ctx.save_for_backward(x, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        check(lib.srk_rownorm_backward(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(dx), x.shape[0], x.shape[1], stream_ptr()),
              "srk_rownorm_backward")
        return dx, None


def row_norm(x, eps=1e-5):
    """nn.InstanceNorm1d(F) with its defaults on a [B, F] tensor."""
    if x.dim() != 2:
        raise RuntimeError("row_norm expects a [B, F] tensor, got shape %s" % (tuple(x.shape),))
    return _RowNorm.apply(x, float(eps))


class _UpsampleNearest(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r):
        lib = _lib.load()
        require_cuda(x)
        x = to_nhwc(x)
        n, c, h, w = x.shape
        y = _empty_cl(n, c, h * r, w * r, x)
        check(lib.srk_upsample_nearest_forward(ptr(x), ptr(y), n, h, w, c, r, stream_ptr()), "srk_upsample_nearest_forward")
        ctx.r = r
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        r = ctx.r
        dy = _dense(dy)
        n, c, hr, wr = dy.shape
        dx = _empty_cl(n, c, hr // r, wr // r, dy)
        check(lib.srk_upsample_nearest_backward(ptr(dy), ptr(dx), n, hr // r, wr // r, c, r, stream_ptr()),
              "srk_upsample_nearest_backward")
        return dx, None


def upsample_nearest(x, r):
    """torch.nn.Upsample(scale_factor=r, mode='nearest') (base_networks.py:206)."""
    return _UpsampleNearest.apply(x, int(r))


def max_pool2x2(x):
    """nn.MaxPool2d(2, 2) of vgg19.features[4] (srgan.py:84-90).  No-grad only: the reference feeds the VGG loss
    detached tensors (srgan.py:302-305)."""
    if grad_enabled_for(x):
        raise RuntimeError("max_pool2x2 has no backward (the reference's VGG loss carries no gradient, srgan.py:302-305); "
                           "call it under torch.no_grad() or on detached tensors")
    lib = _lib.load()
    require_cuda(x)
    x = to_nhwc(x)
    n, c, h, w = x.shape
    if h < 2 or w < 2:
        raise RuntimeError("max_pool2x2: input %s too small" % (tuple(x.shape),))
    y = _empty_cl(n, c, h // 2, w // 2, x)
    check(lib.srk_maxpool2x2_forward(ptr(x), ptr(y), n, h, w, c, stream_ptr()), "srk_maxpool2x2_forward")
    return y


class _MaxPool2x2(torch.autograd.Function):
    """MaxPool2d(2, 2) with its gradient (srk_maxpool2x2_backward).  Only x is saved: the backward kernel recomputes
    each window's winner.  When x is the output of a fused conv + ReLU and the backward runs inside
    premasked_gradients(), dx leaves already multiplied by that ReLU's mask and carries the mark (see PREMASK)."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        require_cuda(x)
        x = to_nhwc(x)
        n, c, h, w = x.shape
        if h < 2 or w < 2:
            raise RuntimeError("max_pool2x2_train: input %s too small" % (tuple(x.shape),))
        y = _empty_cl(n, c, h // 2, w // 2, x)
        check(lib.srk_maxpool2x2_forward(ptr(x), ptr(y), n, h, w, c, stream_ptr()), "srk_maxpool2x2_forward")
        ctx.x_relu_out = _is_relu_output(x)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, = ctx.saved_tensors
        dy = to_nhwc(dy if (_is_nchw_dense(dy) or _is_nhwc_dense(dy)) else dy.contiguous())
        n, c, h, w = x.shape
        dx = _empty_cl(n, c, h, w, dy)
        premask = ctx.x_relu_out and _premask_on() and not x.retains_grad
        check(lib.srk_maxpool2x2_backward(ptr(x), ptr(dy), ptr(dx), n, h, w, c, int(premask), stream_ptr()),
              "srk_maxpool2x2_backward")
        if premask:
            dx._srk_premasked = (x.data_ptr(), _ver(dx))
            PREMASK_STATS["masked_dx"] += 1
        return dx


def max_pool2x2_train(x):
    """nn.MaxPool2d(2, 2) with a backward: the pool of a VGG head whose loss trains (perceptual_loss).  max_pool2x2 stays
    the no-grad form."""
    return _MaxPool2x2.apply(x)


def perceptual_loss(pred, target, extractor, normalize=True, criterion='mse'):
    """The VGG feature loss of SRGAN (srgan.py:301-305) as a term that trains: MSE(extractor.extract(norm(pred)),
    extractor.extract(norm(target))), norm = utils.norm(vgg=True) when `normalize`; a 0-dim fp32 device tensor with the
    seed contract of the losses, _declare_seed (it IS ops.mse_loss on the two feature maps).  The gradient flows to pred
    only.  Both operands run the same kernels -- the training forward of the head, the target's without a graph -- so
    equal inputs give a loss of exactly 0 and a zero gradient.
    pred / target: [N, 3, H, W]; extractor: models.FeatureExtractor.  criterion: 'mse' (SRGAN) or 'l1' (ESRGAN: ops.l1_loss
    on the two feature maps, the same contract)."""
    from . import utils
    if criterion not in ('mse', 'l1'):
        raise ValueError("perceptual_loss: criterion = %r is neither 'mse' nor 'l1'" % (criterion,))
    for name, t in (("pred", pred), ("target", target)):
        if t.dim() != 4 or t.shape[1] != 3:
            raise ValueError("perceptual_loss: %s must be [N, 3, H, W] (the VGG head reads RGB), got shape %s"
                             % (name, tuple(t.shape)))
    if pred.shape != target.shape:
        raise ValueError("perceptual_loss: pred %s vs target %s" % (tuple(pred.shape), tuple(target.shape)))
    with torch.no_grad():
        t = target.detach()
        real = extractor.extract(utils.norm(t, vgg=True) if normalize else t, grad=True)
    fake = extractor.extract(utils.norm(pred, vgg=True) if normalize else pred, grad=True)
    return mse_loss(fake, real) if criterion == 'mse' else l1_loss(fake, real)


# ---- the multi-layer VGG feature loss (Real-ESRGAN's; csrc/vgg_tap.hip) -------------------------------
REALESRGAN_VGG_LAYERS = (('conv1_2', 0.1), ('conv2_2', 0.1), ('conv3_4', 1.0), ('conv4_4', 1.0), ('conv5_4', 1.0))


def vgg_conv_names(cfg):
    """{'conv{k}_{j}': torchvision index} of a VGG configuration (numbers = conv3x3 channels, each followed by its ReLU;
    'M' = the pool that ends block k): for vgg19, conv1_2 -> 2, conv2_2 -> 7, conv3_4 -> 16, conv4_4 -> 25, conv5_4 -> 34."""
    names, idx, k, j = {}, 0, 1, 0
    for v in cfg:
        if v == 'M':
            idx, k, j = idx + 1, k + 1, 0
        else:
            j += 1
            names['conv%d_%d' % (k, j)] = idx
            idx += 2
    return names


def vgg_layer_plan(layer_weights, cfg):
    """The taps of a layer_weights mapping (or a sequence of (name, weight) pairs), checked: [(name, index, weight)] in the
    order of the head, weight-0 layers dropped.  ValueError, naming the culprit: a name that is no conv of `cfg`, a
    duplicate, a negative or non-finite weight, nothing left."""
    names = vgg_conv_names(cfg)
    pairs = list(layer_weights.items()) if hasattr(layer_weights, "items") else [tuple(p) for p in layer_weights]
    seen, plan = set(), []
    for name, weight in pairs:
        if name not in names:
            raise ValueError("vgg_layers: %r is not a VGG19 conv layer (conv1_1 .. conv5_4; relu* and pool* taps are not "
                             "built)" % (name,))
        if name in seen:
            raise ValueError("vgg_layers: %r is named twice" % (name,))
        seen.add(name)
        try:
            weight = float(weight)
        except (TypeError, ValueError):
            raise ValueError("vgg_layers: the weight %r of %r is not a number" % (weight, name))
        if not 0.0 <= weight < float("inf"):
            raise ValueError("vgg_layers: the weight %r of %r is not a non-negative finite number" % (weight, name))
        if weight > 0.0:
            plan.append((name, names[name], weight))
    if not plan:
        raise ValueError("vgg_layers: no layer with a positive weight")
    return sorted(plan, key=lambda p: p[1])


class _VggTap(torch.autograd.Function):
    """One tapped layer (srk_vgg_tap_forward / _backward, one launch each): a, b the pre-activation maps of prediction and
    target; writes row `row` of the term's workspace and returns (token, ya, yb) -- the token ties the row into
    _VggTapFinish, ya / yb are what the head runs behind the tap (None for VGG_TAP_LAST).  a and b are what the backward
    keeps.  The gradient goes to a only; the seed contract of the losses holds per tap (_declare_seed)."""

    @staticmethod
    def forward(ctx, a, b, mode, weight, row, rows, ws):
        lib = _lib.load()
        require_cuda(a, b)
        if a.dim() != 4 or a.shape != b.shape:
            raise RuntimeError("vgg_tap: maps %s and %s must be equal 4-D NCHW shapes" % (tuple(a.shape), tuple(b.shape)))
        a, b = _nhwc(a), _nhwc(b.detach())
        n, c, h, w = a.shape
        ya = yb = None
        if mode == _lib.VGG_TAP_POOL:
            if h < 2 or w < 2:
                raise RuntimeError("vgg_tap: a %d x %d map has no 2 x 2 window to pool" % (h, w))
            ya, yb = _empty_cl(n, c, h // 2, w // 2, a), _empty_cl(n, c, h // 2, w // 2, a)
        elif mode == _lib.VGG_TAP_RELU:
            ya, yb = _empty_cl(n, c, h, w, a), _empty_cl(n, c, h, w, a)
        check(lib.srk_vgg_tap_forward(ptr(a), ptr(b), n, h, w, c, mode, float(weight), int(row), int(rows), ptr(ws), ptr(ya),
                                      ptr(yb), stream_ptr()), "srk_vgg_tap_forward")
        ctx.mode, ctx.scale = mode, float(weight) / float(a.numel())
        _declare_seed(ctx)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(a, b)
        token = torch.empty((), dtype=torch.float32, device=a.device)   # (never read: it carries the graph edge)
        if yb is not None:
            ctx.mark_non_differentiable(yb)
        return token, ya, yb

    @staticmethod
    def backward(ctx, g_token, g_ya, g_yb):
        lib = _lib.load()
        a, b = ctx.saved_tensors
        n, c, h, w = a.shape
        mode = ctx.mode if g_ya is not None else _lib.VGG_TAP_LAST   # nothing behind the tap was used
        g_ya = _nhwc(g_ya) if mode != _lib.VGG_TAP_LAST else None
        factor = None
        if g_token is None:
            coeff = 0.0
        elif _is_own_seed(ctx, g_token, a.device):     # c is known on the host: the seed is folded in here
            coeff = ctx.scale * ctx.seed_value
        else:                                          # a foreign gradient multiplies the unseeded c on the device
            coeff, factor = ctx.scale, g_token.to(torch.float32).contiguous()
        da = _empty_cl(n, c, h, w, a)
        check(lib.srk_vgg_tap_backward(ptr(a), ptr(b), ptr(g_ya), n, h, w, c, mode, coeff, ptr(factor), ptr(da),
                                       stream_ptr()), "srk_vgg_tap_backward")
        return da, None, None, None, None, None, None


def vgg_tap(a, b, mode, weight, row, rows, ws):
    """One tap of the multi-layer VGG feature loss: see _VggTap.  mode: _lib.VGG_TAP_POOL / _RELU / _LAST; ws: the uint8
    workspace of srk_vgg_tap_workspace_bytes(rows) bytes that the term's taps share."""
    return _VggTap.apply(a, b, int(mode), float(weight), int(row), int(rows), ws)


class _VggTapFinish(torch.autograd.Function):
    """The rows of the term's workspace added in order (one launch): sum_k w_k * mean_k as a 0-dim fp32 tensor.  The
    backward hands its upstream gradient to every tap as it came, so each tap recognises its own seed."""

    @staticmethod
    def forward(ctx, ws, rows, *tokens):
        lib = _lib.load()
        loss = torch.empty((), dtype=torch.float32, device=ws.device)
        check(lib.srk_vgg_tap_finish(ptr(ws), int(rows), ptr(loss), stream_ptr()), "srk_vgg_tap_finish")
        ctx.k = len(tokens)
        return loss

    @staticmethod
    def backward(ctx, g):
        return (None, None) + (g,) * ctx.k


def vgg_tap_finish(ws, rows, tokens):
    return _VggTapFinish.apply(ws, int(rows), *tokens)


def vgg_feature_loss(pred, target, extractor, layer_weights, normalize=True, criterion='l1'):
    """Real-ESRGAN's feature term: sum_k w_k * L1(f_k(norm(pred)), f_k(norm(target))), f_k the VGG19 map of layer k BEFORE
    its ReLU, as a 0-dim fp32 device tensor with the seed contract of the losses (_declare_seed); ops.weighted_term and
    ops.loss_sum take it like any other.  layer_weights: an ordered mapping {'conv1_2': 0.1, ...} of conv names of
    extractor.VGG19_CFG (vgg_layer_plan says what is refused; a weight of 0 drops the layer).  Prediction and target walk
    the head in lockstep (extractor.tap_walk), the target without a graph on the same kernels, so equal inputs give exactly
    0.0 and a zero gradient; each tapped layer is one fused launch each way (vgg_tap) and one more launch adds the rows.
    The gradient flows to pred only.  Only the L1 criterion is built.  pred / target: [N, 3, H, W]; extractor:
    models.FeatureExtractor reaching the deepest named layer."""
    from . import utils
    if criterion != 'l1':
        raise ValueError("vgg_feature_loss: criterion = %r is not built, only 'l1' is" % (criterion,))
    plan = vgg_layer_plan(layer_weights, extractor.VGG19_CFG)
    for name, t in (("pred", pred), ("target", target)):
        if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 3:
            raise ValueError("vgg_feature_loss: %s must be [N, 3, H, W] (the VGG head reads RGB), got %s"
                             % (name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    if pred.shape != target.shape:
        raise ValueError("vgg_feature_loss: pred %s vs target %s" % (tuple(pred.shape), tuple(target.shape)))
    if plan[-1][1] >= len(extractor.features):
        raise ValueError("vgg_feature_loss: %r is layer %d of the head, the extractor keeps %d (FeatureExtractor("
                         "feature_layer=%d))" % (plan[-1][0], plan[-1][1], len(extractor.features), plan[-1][1]))
    with torch.no_grad():
        t = target.detach()
        b = utils.norm(t, vgg=True) if normalize else t
    a = utils.norm(pred, vgg=True) if normalize else pred
    return extractor.tap_walk(a, b, [(idx, weight) for _, idx, weight in plan])


def grad_enabled_for(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _strides4(t):
    """Element strides (n, c, h, w) of a [N,C,H,W] tensor in any dense-or-view layout, as a ctypes array."""
    return (ctypes.c_int64 * 4)(*[int(v) for v in t.stride()])


def psnr(pred, gt):
    """utils.PSNR (utils.py:208-216) on the device: returns (psnr, mse) as 0-dim device tensors, no host sync.
    pred / gt: [N,C,H,W] or [C,H,W] CUDA tensors of any strides (channels_last net outputs, NCHW targets, crops)."""
    lib = _lib.load()
    require_cuda(pred, gt)
    if pred.shape != gt.shape:
        raise RuntimeError("psnr: pred %s vs gt %s" % (tuple(pred.shape), tuple(gt.shape)))
    p = pred.detach()
    g = gt.detach()
    if p.dim() == 3:
        p, g = p.unsqueeze(0), g.unsqueeze(0)
    if p.dim() != 4:
        raise RuntimeError("psnr expects [N,C,H,W] or [C,H,W] tensors, got shape %s" % (tuple(pred.shape),))
    n, c, h, w = p.shape
    out = torch.empty(2, dtype=torch.float32, device=p.device)
    ws = torch.empty(int(lib.srk_psnr_workspace_bytes()), dtype=torch.uint8, device=p.device)
    check(lib.srk_psnr(ptr(p), _strides4(p), ptr(g), _strides4(g), n, c, h, w, ptr(out[0:1]), ptr(out[1:2]), ptr(ws),
                       stream_ptr()), "srk_psnr")
    return out[0], out[1]


def ssim(pred, gt, shave=0, domain='float'):
    """SSIM (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, valid positions, fp64 moments) of pred against gt on
    the device, with PSNR and MSE of the same pixels from the same pass: returns (ssim, psnr, mse) as 0-dim device
    tensors, no host sync.  pred / gt: [N,C,H,W] or [C,H,W] CUDA tensors of any strides, read in place.
    shave: pixels cropped from each side of both first.  domain: 'float' -- clamp(pred, 0, 1) against gt, what psnr()
    compares; 'u8' -- both quantised like to_u8_image, the picture save_img writes; 'y8' -- that picture's Pillow luma
    (three channels), or 'u8' for one channel.  include/srk.h: srk_ssim."""
    lib = _lib.load()
    require_cuda(pred, gt)
    if pred.shape != gt.shape:
        raise RuntimeError("ssim: pred %s vs gt %s" % (tuple(pred.shape), tuple(gt.shape)))
    if domain not in _lib.SSIM_DOMAINS:
        raise RuntimeError("ssim: domain %r is not one of %s" % (domain, sorted(_lib.SSIM_DOMAINS)))
    p = pred.detach()
    g = gt.detach()
    if p.dim() == 3:
        p, g = p.unsqueeze(0), g.unsqueeze(0)
    if p.dim() != 4:
        raise RuntimeError("ssim expects [N,C,H,W] or [C,H,W] tensors, got shape %s" % (tuple(pred.shape),))
    n, c, h, w = p.shape
    shave = int(shave)
    if shave < 0 or min(h, w) - 2 * shave < 11:
        raise RuntimeError("ssim: planes of %d x %d with shave %d leave %d x %d, under the 11 x 11 window"
                           % (h, w, shave, h - 2 * shave, w - 2 * shave))
    if domain == 'y8' and c not in (1, 3):
        raise RuntimeError("ssim: domain 'y8' takes 1 or 3 channels, got %d" % c)
    out = torch.empty(3, dtype=torch.float32, device=p.device)
    ws = torch.empty(int(lib.srk_ssim_workspace_bytes()), dtype=torch.uint8, device=p.device)
    check(lib.srk_ssim(ptr(p), _strides4(p), ptr(g), _strides4(g), n, c, h, w, shave, _lib.SSIM_DOMAINS[domain],
                       ptr(out[0:1]), ptr(out[1:2]), ptr(out[2:3]), ptr(ws), stream_ptr()), "srk_ssim")
    return out[0], out[1], out[2]


def _channel_affine_raw(x, sub, div, clamp01=False):
    """y = (x - sub[c]) / div[c] per channel (utils.norm / utils.denorm, utils.py:219-239), same storage layout as x
    ([C,H,W] / [B,C,H,W] NCHW-contiguous or channels_last); bit-equal to torchvision's Normalize."""
    lib = _lib.load()
    require_cuda(x)
    if x.dim() not in (3, 4):
        raise RuntimeError("channel_affine expects [C,H,W] or [B,C,H,W], got shape %s" % (tuple(x.shape),))
    c = x.shape[-3]
    if len(sub) < c or len(div) < c:
        raise RuntimeError("channel_affine: %d channels but only %d constants" % (c, min(len(sub), len(div))))
    x4 = x if x.dim() == 4 else x.unsqueeze(0)
    if _is_nchw_dense(x4):
        xs = x4 if x4.is_contiguous() else x4.contiguous()
        inner = x.shape[-1] * x.shape[-2]
    elif _is_nhwc_dense(x4):
        xs, inner = x4, 1
    else:
        xs = x4.contiguous()
        inner = x.shape[-1] * x.shape[-2]
    y = torch.empty_like(xs)
    if y.stride() != xs.stride():
        raise RuntimeError("channel_affine: internal layout mismatch")
    fa = (ctypes.c_float * c)(*[float(v) for v in sub[:c]])
    fb = (ctypes.c_float * c)(*[float(v) for v in div[:c]])
    check(lib.srk_channel_affine(ptr(xs), ptr(y), xs.numel(), c, inner, fa, fb, int(bool(clamp01)), stream_ptr()),
          "srk_channel_affine")
    return y if x.dim() == 4 else y[0]


class _ChannelAffine(torch.autograd.Function):
    """(x - sub[c]) / div[c] with its gradient dy / div[c] (the same kernel with sub = 0)."""

    @staticmethod
    def forward(ctx, x, sub, div):
        ctx.div = tuple(float(v) for v in div)
        return _channel_affine_raw(x, sub, div)

    @staticmethod
    def backward(ctx, dy):
        return _channel_affine_raw(dy, (0.0,) * len(ctx.div), ctx.div), None, None


def channel_affine(x, sub, div, clamp01=False):
    """utils.norm / utils.denorm (utils.py:219-239).  Differentiable like the reference's tensor arithmetic when x
    requires grad; the clamped form ((img + 1) / 2).clamp(0, 1) is only available without a graph (the reference uses it
    on detached images when it saves results) and raises otherwise instead of dropping the gradient silently."""
    if torch.is_grad_enabled() and x.requires_grad:
        if clamp01:
            raise RuntimeError("channel_affine(clamp01=True) has no backward: call it on a detached tensor "
                               "(utils.denorm of an image that requires grad)")
        return _ChannelAffine.apply(x, tuple(sub), tuple(div))
    return _channel_affine_raw(x, sub, div, clamp01)


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act, slope):
        lib = _lib.load()
        require_cuda(x, weight, bias)
        x = x.contiguous()
        b, fin = x.shape
        fout = weight.shape[0]
        y = torch.empty((b, fout), dtype=torch.float32, device=x.device)
        check(lib.srk_linear_forward(ptr(x), ptr(weight), ptr(bias), ptr(y), b, fin, fout, act, slope, stream_ptr()),
              "srk_linear_forward")
        ctx.act, ctx.slope = act, slope
        ctx.weight_ref, ctx.bias_ref = weight, bias
        ctx.save_for_backward(x, weight, y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, weight, y = ctx.saved_tensors
        dy = dy.contiguous()
        b, fin = x.shape
        fout = weight.shape[0]
        if y is not None:
            dz = torch.empty_like(dy)
            check(lib.srk_act_backward(ptr(dy), ptr(y), ptr(dz), dy.numel(), fout, ctx.act, ctx.slope, None, 0, None,
                                       stream_ptr()), "srk_act_backward")
            dy = dz
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        has_bias = ctx.bias_ref is not None
        wacc = getattr(ctx.weight_ref, "_srk_grad", None)
        bacc = getattr(ctx.bias_ref, "_srk_grad", None) if has_bias else None
        need_w = ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2])
        if not need_w:   # frozen parameters (trainers.srgan_step(prune_dead_grads=True)): data gradient only
            if dx is not None:
                check(lib.srk_linear_backward(ptr(x), ptr(weight), ptr(dy), ptr(dx), None, None, b, fin, fout, 0.0,
                                              stream_ptr()), "srk_linear_backward")
            return dx, None, None, None, None
        if wacc is not None and (not has_bias or bacc is not None):
            check(lib.srk_linear_backward(ptr(x), ptr(weight), ptr(dy), ptr(dx), ptr(wacc), ptr(bacc), b, fin, fout,
                                          1.0, stream_ptr()), "srk_linear_backward")
            return dx, None, None, None, None
        dw = torch.empty_like(weight)
        db = torch.empty(fout, dtype=torch.float32, device=x.device) if has_bias else None
        check(lib.srk_linear_backward(ptr(x), ptr(weight), ptr(dy), ptr(dx), ptr(dw), ptr(db), b, fin, fout, 0.0,
                                      stream_ptr()), "srk_linear_backward")
        return dx, dw, db, None, None


def linear(x, weight, bias=None, act=ACT_NONE, slope=0.0):
    """nn.Linear + activation of DenseBlock (base_networks.py:7,26-35). PReLU is applied unfused."""
    return _Linear.apply(x, weight, bias, int(act), float(slope))


_INTERP = {"nearest": _lib.INTERP_NEAREST, "bilinear": _lib.INTERP_BILINEAR, "bicubic": _lib.INTERP_BICUBIC}


def img_interp(imgs, scale_factor, interpolation="bicubic"):
    """utils.img_interp (utils.py:242-269) on the GPU: uint8 quantisation, Pillow's two-pass 8-bit resampling and
    the /255 of ToTensor in three small kernels, bit-exact with the reference's PIL round trip.  `imgs` is a
    [B,C,H,W] or [C,H,W] CUDA tensor; returns a dense NCHW tensor of size int(H*s) x int(W*s) like the reference."""
    require_cuda(imgs)
    if interpolation not in _INTERP:
        raise ValueError("interpolation must be one of %s" % sorted(_INTERP))
    squeeze = imgs.dim() == 3
    x = imgs.unsqueeze(0) if squeeze else imgs
    if x.dim() != 4:
        raise RuntimeError("img_interp expects a [B,C,H,W] or [C,H,W] tensor, got shape %s" % (tuple(imgs.shape),))
    x = x.detach().float().contiguous()
    n, c, h, w = x.shape
    oh, ow = int(h * scale_factor), int(w * scale_factor)
    if oh <= 0 or ow <= 0:
        raise RuntimeError("img_interp: empty output for scale %r" % (scale_factor,))
    lib = _lib.load()
    flt = _INTERP[interpolation]
    y = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    nbytes = int(lib.srk_img_interp_workspace_bytes(n, c, h, w, oh, ow, flt))
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=x.device)
    check(lib.srk_img_interp(ptr(x), ptr(y), n, c, h, w, oh, ow, flt, ptr(ws), ws.numel(), stream_ptr()), "srk_img_interp")
    return y[0] if squeeze else y



# ------------------------------------------------------------------------------------------------
# The colour tail of test_single / test (edsr.py:276-322): 8-bit images on the device, bit-exact with Pillow
# ------------------------------------------------------------------------------------------------
def _require_u8(what, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("%s runs on GPU tensors (got a %s tensor); there is no CPU fallback" % (what, t.device))
        if t.device.index is not None and t.device.index != torch.cuda.current_device():
            raise RuntimeError("%s: tensor on %s but the current device is cuda:%d" % (what, t.device, torch.cuda.current_device()))
        if t.dtype != torch.uint8:
            raise RuntimeError("%s expects uint8 tensors (got %s)" % (what, t.dtype))


def _picture_chw(what, x, hw=None):
    """The picture x ([C,H,W] or [1,C,H,W], C = 1 or 3; with hw = (H, W): fp32 and of that size) as a detached [C,H,W]
    view.  `what`: the sentence of the error, up to ', got ...'."""
    require_cuda(x)
    v = x.detach()
    if v.dim() == 4 and v.shape[0] == 1:
        v = v[0]
    if v.dim() != 3 or v.shape[0] not in (1, 3) or (hw is not None and (v.dtype != torch.float32 or tuple(v.shape[1:]) != hw)):
        raise RuntimeError("%s, got %s %s" % (what, x.dtype, tuple(x.shape)))
    return v


def _f32_out(what, shape, device, out):
    """The fp32 destination of `shape`: `out` checked, or allocated when None."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
        raise RuntimeError("%s: out must be a dense fp32 [%s] tensor on %s" % (what, ",".join(str(v) for v in shape), device))
    return out


def _u8_out(what, c, h, w, device, cb=None, cr=None, out=None):
    """The 8-bit destination of a picture of c channels: interleaved uint8 [h,w,c], or with the chroma planes cb / cr
    (uint8 [h,w], c = 1) [h,w,3].  Returns (cb, cr, out): the planes dense, `out` checked, or allocated when None."""
    if (cb is None) != (cr is None):
        raise RuntimeError("%s: cb and cr come together" % what)
    oc = c
    if cb is not None:
        _require_u8(what, cb, cr)
        if cb.device != device or cr.device != device:
            raise RuntimeError("%s: the chroma planes are on %s / %s, the net outputs on %s" % (what, cb.device, cr.device, device))
        if c != 1 or tuple(cb.shape) != (h, w) or tuple(cr.shape) != (h, w):
            raise RuntimeError("%s: chroma planes must be [%d,%d] and go with a one-channel output (got C = %d, cb %s, cr %s)"
                               % (what, h, w, c, tuple(cb.shape), tuple(cr.shape)))
        cb, cr, oc = cb.contiguous(), cr.contiguous(), 3
    if out is None:
        out = torch.empty((h, w, oc), dtype=torch.uint8, device=device)
    elif tuple(out.shape) != (h, w, oc) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != device:
        raise RuntimeError("%s: out must be a dense uint8 [%d,%d,%d] tensor on %s" % (what, h, w, oc, device))
    return cb, cr, out


def rgb_to_ycc_planes(img_u8_hwc, y_float=False):
    """One pass of k_rgb_to_ycc over an interleaved 8-bit RGB image [H,W,3] (a row-strided view is read in place; pixels
    must be dense): returns (y, cbcr) with cbcr uint8 [2,H,W] planar -- what resize_u8 takes -- and y uint8 [H,W] or,
    with y_float, the fp32 plane Y / 255 that ToTensor() makes of the Y image."""
    _require_u8("rgb_to_ycbcr_u8", img_u8_hwc)
    x = img_u8_hwc
    if x.dim() != 3 or x.shape[2] != 3:
        raise RuntimeError("rgb_to_ycbcr_u8 expects an interleaved [H,W,3] image, got shape %s" % (tuple(x.shape),))
    h, w = int(x.shape[0]), int(x.shape[1])
    if h == 0 or w == 0:
        raise RuntimeError("rgb_to_ycbcr_u8: empty image %s" % (tuple(x.shape),))
    if x.stride(2) != 1 or x.stride(1) != 3 or (h > 1 and x.stride(0) < 3 * w):
        x = x.contiguous()
    row_stride = int(x.stride(0)) if h > 1 else 3 * w
    y = torch.empty((h, w), dtype=torch.float32 if y_float else torch.uint8, device=x.device)
    cbcr = torch.empty((2, h, w), dtype=torch.uint8, device=x.device)
    check(_lib.load().srk_rgb_to_ycc_u8(ptr(x), row_stride, h, w, ptr(y) if y_float else None, None if y_float else ptr(y),
                                        ptr(cbcr), stream_ptr()), "srk_rgb_to_ycc_u8")
    return y, cbcr


def rgb_to_ycbcr_u8(img_u8_hwc, y_float=False):
    """Image.convert('YCbCr').split() of an interleaved 8-bit RGB image [H,W,3] on the device, bit-exact with Pillow:
    (y, cb, cr), uint8 [H,W] each; with y_float, y is the fp32 plane Y / 255 instead (see rgb_to_ycc_planes)."""
    y, cbcr = rgb_to_ycc_planes(img_u8_hwc, y_float)
    return y, cbcr[0], cbcr[1]


def ycbcr_to_rgb_u8(y, cb, cr):
    """Image.merge('YCbCr', [y, cb, cr]).convert('RGB') on the device (k_ycc_to_rgb), bit-exact with Pillow: interleaved
    uint8 [H,W,3].  cb / cr: uint8 [H,W].  y: uint8 [H,W], or the fp32 output of a Y-channel net ([H,W], [1,H,W] or
    [1,1,H,W], any strides), which is quantised like ToPILImage after clamp(0, 1) inside the kernel."""
    h, w = int(cb.shape[-2]), int(cb.shape[-1])
    cb, cr, out = _u8_out("ycbcr_to_rgb_u8", 1, h, w, cb.device, cb, cr)
    if y.numel() != h * w or tuple(y.shape[-2:]) != (h, w):
        raise RuntimeError("ycbcr_to_rgb_u8: y %s does not match the chroma planes %s" % (tuple(y.shape), (h, w)))
    lib = _lib.load()
    if y.dtype == torch.uint8:
        _require_u8("ycbcr_to_rgb_u8", y)
        y = y.reshape(h, w).contiguous()
        rc = lib.srk_ycc_to_rgb_u8(None, 0, 0, ptr(y), ptr(cb), ptr(cr), ptr(out), h, w, stream_ptr())
    else:
        require_cuda(y)
        y = y.detach()
        rc = lib.srk_ycc_to_rgb_u8(ptr(y), int(y.stride(-2)), int(y.stride(-1)), None, ptr(cb), ptr(cr), ptr(out), h, w,
                                   stream_ptr())
    check(rc, "srk_ycc_to_rgb_u8")
    return out


def to_u8_image(x):
    """ToPILImage()(x.clamp(0, 1)) as an array (edsr.py:305-306), on the device (k_to_u8): fp32 [C,H,W] or [1,C,H,W]
    of any strides (a channels-last net output is read in place), C = 1 or 3 -> interleaved uint8 [H,W,C], each byte
    (uint8)(clamp(x, 0, 1) * 255) with the fp32 product truncated; NaN gives 0."""
    x = _picture_chw("to_u8_image expects a [C,H,W] or [1,C,H,W] tensor with C = 1 or 3", x)
    c, h, w = (int(v) for v in x.shape)
    out = _u8_out("to_u8_image", c, h, w, x.device)[2]
    check(_lib.load().srk_float_to_u8_image(ptr(x), int(x.stride(0)), int(x.stride(1)), int(x.stride(2)), ptr(out), c, h, w,
                                            stream_ptr()), "srk_float_to_u8_image")
    return out


def resize_u8(planes_u8, oh, ow, interpolation="bicubic", out_float=False, out=None):
    """Image.resize((ow, oh)) of 8-bit planes [P,H,W] (any strides: an interleaved [H,W,C] image is read in place through
    .permute(2, 0, 1)) on the device: srk_img_resize_u8, bit-exact with Pillow.  Returns uint8 [P,oh,ow], or with
    out_float the fp32 planes value / 255 (ToTensor); an unchanged size makes that the plain ToTensor of the image.
    out: a dense tensor of that shape and type to write into (a slice of a larger buffer along the first axis is one)."""
    _require_u8("resize_u8", planes_u8)
    if planes_u8.dim() != 3:
        raise RuntimeError("resize_u8 expects [P,H,W] planes, got shape %s" % (tuple(planes_u8.shape),))
    if interpolation not in ("bicubic", "bilinear", "box"):
        raise ValueError("resize_u8: interpolation must be 'bicubic', 'bilinear' or 'box'")
    p, h, w = (int(v) for v in planes_u8.shape)
    lib = _lib.load()
    flt = INTERP_BOX if interpolation == "box" else _INTERP[interpolation]
    y = out
    if y is None:
        y = torch.empty((p, oh, ow), dtype=torch.float32 if out_float else torch.uint8, device=planes_u8.device)
    elif tuple(y.shape) != (p, oh, ow) or y.dtype != (torch.float32 if out_float else torch.uint8) or not y.is_contiguous() \
            or y.device != planes_u8.device:
        raise RuntimeError("resize_u8: out must be a dense %s [%d,%d,%d] tensor on %s"
                           % ("fp32" if out_float else "uint8", p, oh, ow, planes_u8.device))
    nbytes = max(int(lib.srk_img_resize_u8_workspace_bytes(p, h, w, oh, ow, flt)), 256)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=planes_u8.device)
    st = [int(v) for v in planes_u8.stride()]
    check(lib.srk_img_resize_u8(ptr(planes_u8), st[0], st[1], st[2], ptr(y), int(out_float), p, h, w, oh, ow, flt, ptr(ws), nbytes,
                                stream_ptr()), "srk_img_resize_u8")
    return y


def _require_f64(what, name, t, shape):
    if not t.is_cuda:
        raise RuntimeError("%s runs on GPU tensors (got %s on %s); there is no CPU fallback" % (what, name, t.device))
    if t.dtype != torch.float64 or tuple(t.shape) != tuple(shape):
        raise RuntimeError("%s: %s must be an fp64 %s tensor, got %s %s" % (what, name, list(shape), t.dtype, tuple(t.shape)))
    return t.contiguous()


def blur_u8(x, weights):
    """Per-patch blur of 8-bit patches x [B,C,H,W] under the fp64 tables weights [B,K,K] (K odd, 3 <= K <= 21, H, W >
    K // 2) on the device: srk_blur_u8.  Each output byte is floor(clamp(sum, 0, 255) + 0.5) of the fp64 sum of its K x K
    taps in row-major order, borders mirrored without repeating the edge pixel; the delta table returns x."""
    _require_u8("blur_u8", x)
    if x.dim() != 4 or weights.dim() != 3:
        raise RuntimeError("blur_u8 expects x [B,C,H,W] and weights [B,K,K], got %s and %s" % (tuple(x.shape), tuple(weights.shape)))
    b, c, h, w = (int(v) for v in x.shape)
    k = int(weights.shape[-1])
    weights = _require_f64("blur_u8", "weights", weights, (b, k, k))
    x = x.contiguous()
    y = torch.empty_like(x)
    check(_lib.load().srk_blur_u8(ptr(x), ptr(y), ptr(weights), c, b, h, w, k, stream_ptr()), "srk_blur_u8")
    return y


def noise_u8(x, sigma, seed):
    """Additive Gaussian noise on 8-bit patches x [B,...] with one standard deviation per patch (sigma fp64 [B], in 8-bit
    levels) on the device: srk_noise_u8.  Returns fp32 floor(x + sigma * z + 0.5) clamped to [0, 255] and divided by 255;
    z from Philox4x32-10 under the 64-bit `seed` on the element's index, Box-Muller in fp64.  sigma 0 gives x / 255."""
    _require_u8("noise_u8", x)
    if x.dim() < 1 or x.numel() == 0:
        raise RuntimeError("noise_u8 expects a non-empty [B,...] tensor, got shape %s" % (tuple(x.shape),))
    b = int(x.shape[0])
    sigma = _require_f64("noise_u8", "sigma", sigma, (b,))
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("noise_u8: seed must fit 64 bits (got %d)" % seed)
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(_lib.load().srk_noise_u8(ptr(x), ptr(y), ptr(sigma), seed, b, x.numel() // b, stream_ptr()), "srk_noise_u8")
    return y


JPEG_SUBSAMPLING = {"4:2:0": 1, "420": 1, 420: 1, "4:4:4": 0, "444": 0, 444: 0}


def jpeg_subsampling(value):
    """'4:2:0' / '420' / 420 -> 1, '4:4:4' / '444' / 444 -> 0 (srk_jpeg_u8's subsampling); anything else is a ValueError."""
    try:
        return JPEG_SUBSAMPLING[value]
    except (KeyError, TypeError):
        raise ValueError("jpeg subsampling must be '4:2:0' or '4:4:4' (got %r)" % (value,))


def jpeg_u8(x, quality, subsampling='4:2:0', color=True, out_float=False):
    """JPEG artefacts on 8-bit patches x [B,C,H,W] (C 1 or 3) on the device: srk_jpeg_u8, every patch compressed at its
    quality and decoded again, byte for byte what Pillow's save(quality=q, subsampling=...) and open give (libjpeg's integer
    baseline path).  quality: an integer tensor [B] (or a Python int for all patches), 1..100, and 0 = leave
    the patch as it is; a tensor's values beyond that range act as libjpeg clamps them, below 1 as 1 and above 100 as 100.  color: the planes are R, G, B (needs C = 3); else they are Y, Cb, Cr, or with C = 1 a grey
    picture.  Returns uint8, or with out_float the fp32 bytes / 255."""
    _require_u8("jpeg_u8", x)
    if x.dim() != 4 or x.numel() == 0:
        raise RuntimeError("jpeg_u8 expects a non-empty x [B,C,H,W], got shape %s" % (tuple(x.shape),))
    b, c, h, w = (int(v) for v in x.shape)
    sub = jpeg_subsampling(subsampling)
    if isinstance(quality, torch.Tensor):
        if quality.is_floating_point() or quality.dtype == torch.bool or tuple(quality.shape) != (b,):
            raise RuntimeError("jpeg_u8: quality must be an integer tensor [%d] or an int, got %s %s"
                               % (b, quality.dtype, tuple(quality.shape)))
        q = quality.to(device=x.device, dtype=torch.float64)      # (not inspected: a look would wait for the device)
    else:
        if int(quality) != quality or not 0 <= quality <= 100:
            raise ValueError("jpeg_u8: quality must be a whole number in 0..100, 0: not compressed (got %r)" % (quality,))
        q = torch.full((b,), float(int(quality)), dtype=torch.float64, device=x.device)
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.float32 if out_float else torch.uint8, device=x.device)
    check(_lib.load().srk_jpeg_u8(ptr(x), ptr(y), ptr(q), c, b, h, w, sub, int(bool(color)), int(bool(out_float)),
                                  stream_ptr()), "srk_jpeg_u8")
    return y


def noise_u8_bytes(x, sigma, seed):
    """noise_u8 with the clamped 8-bit level itself as the result (srk_noise_u8_bytes): bytes / 255 are noise_u8's bits."""
    _require_u8("noise_u8_bytes", x)
    if x.dim() < 1 or x.numel() == 0:
        raise RuntimeError("noise_u8_bytes expects a non-empty [B,...] tensor, got shape %s" % (tuple(x.shape),))
    b = int(x.shape[0])
    sigma = _require_f64("noise_u8_bytes", "sigma", sigma, (b,))
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("noise_u8_bytes: seed must fit 64 bits (got %d)" % seed)
    x = x.contiguous()
    y = torch.empty_like(x)
    check(_lib.load().srk_noise_u8_bytes(ptr(x), ptr(y), ptr(sigma), seed, b, x.numel() // b, stream_ptr()),
          "srk_noise_u8_bytes")
    return y


# ---- Real-ESRGAN's second-order degradation (data.Degradation2) ------------------------------------
INTERP_BOX, POISSON_KT, USM_MAX_K = _lib.INTERP_BOX, _lib.POISSON_KT, _lib.USM_MAX_K
NOISE2_OFF, NOISE2_GAUSS, NOISE2_POISSON = _lib.NOISE2_OFF, _lib.NOISE2_GAUSS, _lib.NOISE2_POISSON
BLUR_KINDS = {"gauss": _lib.BLUR_GAUSS, "ggauss": _lib.BLUR_GGAUSS, "plateau": _lib.BLUR_PLATEAU, "sinc": _lib.BLUR_SINC}
POISSON_PEAK = 256.0                                                    # the chain's fixed peak (not in the header)


def blur_table(kind, K, s1=1.0, s2=1.0, theta=0.0, beta=1.0, cutoff=1.0):
    """srk_blur_table_host: the normalised K x K fp64 table (numpy) of kind 'gauss', 'ggauss', 'plateau' or 'sinc', K odd
    in 7..21, for blur_u8 to take as it is.  Made on the host; needs no GPU."""
    if kind not in BLUR_KINDS:
        raise ValueError("blur_table: kind must be one of %s (got %r)" % (sorted(BLUR_KINDS), kind))
    K = int(K)
    buf = (ctypes.c_double * (K * K if K > 0 else 1))()
    check(_lib.load().srk_blur_table_host(BLUR_KINDS[kind], K, float(s1), float(s2), float(theta), float(beta),
                                          float(cutoff), buf), "srk_blur_table_host")
    return np.frombuffer(buf, np.float64).reshape(K, K)


def poisson_cdf(peak=POISSON_PEAK, KT=POISSON_KT):
    """srk_poisson_cdf_host: the inversion table cdf[256][KT] (fp64 numpy) that noise2_u8 reads, cdf[L][k] = P(Pois(L * peak
    / 255) <= k), last column 1.0.  Made on the host; needs no GPU."""
    out = np.empty((256, int(KT)), np.float64)
    check(_lib.load().srk_poisson_cdf_host(float(peak), int(KT), ctypes.c_void_p(out.ctypes.data)), "srk_poisson_cdf_host")
    return out


def usm_table(K=USM_MAX_K, sigma=0.0):
    """srk_usm_table_host: the normalised K-tap Gaussian (fp64 numpy) of usm_u8; sigma 0 means cv2's rule (8.0 at K = 51)."""
    K = int(K)
    buf = (ctypes.c_double * max(K, 1))()
    check(_lib.load().srk_usm_table_host(K, float(sigma), buf), "srk_usm_table_host")
    return np.frombuffer(buf, np.float64)[:K].copy()


def noise2_u8(x, mode, gray, amount, cdf, seed, stage=0, color=True):
    """The second-order chain's noise on 8-bit patches x [B,C,H,W] (C 1 or 3) on the device: srk_noise2_u8.  mode, gray and
    amount are fp64 [B] per patch: mode 0 leaves the patch, 1 adds Gaussian noise of standard deviation `amount` levels, 2
    Poisson noise scaled by `amount` (k by inversion from `cdf` [256, 448], see poisson_cdf()); gray != 0 draws once per
    pixel for all planes, from the mean of R, G, B (color) or from plane 0 (the Y of Y, Cb, Cr).  `stage` (0, 1, 2) goes into the generator's counter; stage 0 with colour Gaussian noise gives
    noise_u8_bytes' bytes.  Returns uint8 of x's shape; the same inputs give the same bytes."""
    _require_u8("noise2_u8", x)
    if x.dim() != 4 or x.numel() == 0:
        raise RuntimeError("noise2_u8 expects a non-empty x [B,C,H,W], got shape %s" % (tuple(x.shape),))
    b, c, h, w = (int(v) for v in x.shape)
    mode = _require_f64("noise2_u8", "mode", mode, (b,))
    gray = _require_f64("noise2_u8", "gray", gray, (b,))
    amount = _require_f64("noise2_u8", "amount", amount, (b,))
    cdf = _require_f64("noise2_u8", "cdf", cdf, (256, POISSON_KT))
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("noise2_u8: seed must fit 64 bits (got %d)" % seed)
    x = x.contiguous()
    y = torch.empty_like(x)
    check(_lib.load().srk_noise2_u8(ptr(x), ptr(y), ptr(mode), ptr(gray), ptr(amount), ptr(cdf), seed, int(stage), b, c, h, w,
                                    int(bool(color)), stream_ptr()), "srk_noise2_u8")
    return y


def usm_u8(x, g=None, weight=0.5, threshold=10.0):
    """Real-ESRGAN's USMSharp on 8-bit patches x [B,C,H,W] (C 1 or 3, sides > K // 2) on the device: srk_usm_u8.  g: the
    fp64 [K] Gaussian on the device (None: usm_table(), K = 51, sigma 8).  Returns uint8 of x's shape."""
    _require_u8("usm_u8", x)
    if x.dim() != 4 or x.numel() == 0:
        raise RuntimeError("usm_u8 expects a non-empty x [B,C,H,W], got shape %s" % (tuple(x.shape),))
    b, c, h, w = (int(v) for v in x.shape)
    if g is None:
        g = torch.from_numpy(usm_table()).to(x.device)
    k = int(g.numel())
    g = _require_f64("usm_u8", "g", g, (k,))
    x = x.contiguous()
    y = torch.empty_like(x)
    lib = _lib.load()
    nbytes = max(int(lib.srk_usm_u8_workspace_bytes(b, c, h, w)), 256)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    check(lib.srk_usm_u8(ptr(x), ptr(y), ptr(g), k, float(weight), float(threshold), b, c, h, w, ptr(ws), nbytes,
                         stream_ptr()), "srk_usm_u8")
    return y


# ------------------------------------------------------------------------------------------------
# Tiled super-resolution of one picture (tiling.py, csrc/tile.hip): gather the plan's tiles, stitch their outputs
# ------------------------------------------------------------------------------------------------
class TilePlan(object):
    """A tiling.Plan with its table on the device.  The table goes up once, from pinned memory and without waiting for
    the copy; the kernels of every chunk read it there."""

    def __init__(self, plan, device):
        self.plan = plan
        self.nty, self.ntx = len(plan.rows), len(plan.cols)
        host = torch.tensor(plan.table(), dtype=torch.int32).pin_memory()
        self.table = host.to(device, non_blocking=True)
        self._host = host   # (kept until the plan goes: the copy reads it asynchronously)


def _tile_chunk(tp, t0, n):
    t0 = int(t0)
    n = tp.plan.ntiles - t0 if n is None else int(n)
    if t0 < 0 or n < 1 or t0 + n > tp.plan.ntiles:
        raise RuntimeError("tiles %d .. %d are not in a plan of %d tiles" % (t0, t0 + n, tp.plan.ntiles))
    return t0, n


def tile_gather(pic, tp, t0=0, n=None):
    """Tiles t0 .. t0 + n of the plan `tp` (a TilePlan) from the fp32 picture `pic` ([C,H,W] or [1,C,H,W], any strides:
    the planar Y plane of rgb_to_ycc_planes, the planar output of resize_u8 and img_interp's output are read in place),
    C = 1 or 3, as the batch [n,C,th,tw] in channels-last storage the nets take."""
    p = tp.plan
    x = _picture_chw("tile_gather expects an fp32 [C,%d,%d] picture with C = 1 or 3" % (p.H, p.W), pic, (p.H, p.W))
    t0, n = _tile_chunk(tp, t0, n)
    c = int(x.shape[0])
    out = _empty_cl(n, c, p.th, p.tw, x)
    check(_lib.load().srk_tile_gather(ptr(x), int(x.stride(0)), int(x.stride(1)), int(x.stride(2)), c, p.H, p.W, ptr(tp.table),
                                      tp.nty, tp.ntx, p.th, p.tw, t0, n, ptr(out), stream_ptr()), "srk_tile_gather")
    return out


def _stitch_source(what, tiles, tp, t0):
    require_cuda(tiles)
    y = tiles.detach()
    p = tp.plan
    if y.dim() != 4 or y.shape[1] not in (1, 3) or y.dtype != torch.float32 or tuple(y.shape[2:]) != (p.oth, p.otw):
        raise RuntimeError("%s expects fp32 tile outputs [n,C,%d,%d] with C = 1 or 3, got %s %s"
                           % (what, p.oth, p.otw, y.dtype, tuple(tiles.shape)))
    t0, n = _tile_chunk(tp, t0, int(y.shape[0]))
    return y, t0, n, int(y.shape[1])


def tile_stitch(tiles, tp, t0=0, out=None):
    """The owned rectangles of tile outputs `tiles` ([n,C,oth,otw] fp32 of any strides: a channels-last net output is read
    in place; tiles t0 .. t0 + n of the plan) into the fp32 picture `out` [C,OH,OW] (allocated when None; the chunks of
    a plan together write every pixel once).  Returns out."""
    y, t0, n, c = _stitch_source("tile_stitch", tiles, tp, t0)
    p = tp.plan
    out = _f32_out("tile_stitch", (c, p.OH, p.OW), y.device, out)
    check(_lib.load().srk_tile_stitch_f32(ptr(y), int(y.stride(0)), int(y.stride(1)), int(y.stride(2)), int(y.stride(3)), c,
                                          p.oth, p.otw, ptr(tp.table), tp.nty, tp.ntx, t0, n, ptr(out), p.OH, p.OW,
                                          stream_ptr()), "srk_tile_stitch_f32")
    return out


def tile_stitch_u8(tiles, tp, t0=0, out=None, cb=None, cr=None):
    """tile_stitch writing the final 8-bit picture directly: to_u8_image(tile_stitch(...)) without the fp32 picture
    (uint8 [OH,OW,C]), or with the chroma planes cb / cr (uint8 [OH,OW]; C = 1) ycbcr_to_rgb_u8(tile_stitch(...), cb, cr)
    (uint8 [OH,OW,3]); bit-equal to those compositions."""
    y, t0, n, c = _stitch_source("tile_stitch_u8", tiles, tp, t0)
    p = tp.plan
    cb, cr, out = _u8_out("tile_stitch_u8", c, p.OH, p.OW, y.device, cb, cr, out)
    check(_lib.load().srk_tile_stitch_u8(ptr(y), int(y.stride(0)), int(y.stride(1)), int(y.stride(2)), int(y.stride(3)), c,
                                         p.oth, p.otw, ptr(tp.table), tp.nty, tp.ntx, t0, n,
                                         None if cb is None else ptr(cb), None if cr is None else ptr(cr), ptr(out), p.OH, p.OW,
                                         stream_ptr()), "srk_tile_stitch_u8")
    return out


# ------------------------------------------------------------------------------------------------
# x8 geometric self-ensemble (csrc/dihedral.hip): the eight flips / rotations in one launch, their ordered mean in one
# ------------------------------------------------------------------------------------------------
class DihedralVariants(tuple):
    """(even, odd) of dihedral_variants.  `whole` is the one allocation as [8N,C,H,H] when the pictures are square
    (even then odd, so whole[:4N] is even and whole[4N:] is odd), else None."""

    def __new__(cls, even, odd, whole):
        self = super(DihedralVariants, cls).__new__(cls, (even, odd))
        self.even, self.odd, self.whole = even, odd, whole
        return self


def dihedral_variants(x):
    """The eight variants T_k(x), k = 4 m + r, T_k = rot90(flip of the last axis if m, r) of the fp32 pictures x
    ([N,C,H,W] or [C,H,W], any strides, C = 1 or 3) in one launch and one allocation, in the channels-last storage the
    nets take: even [4N,C,H,W] with even[4 n + j] = T_k(x[n]), k = (0, 2, 4, 6)[j], and odd [4N,C,W,H] with
    k = (1, 3, 5, 7)[j].  Returns a DihedralVariants (even, odd); both are views of the allocation."""
    require_cuda(x)
    v = x.detach()
    if v.dim() == 3:
        v = v.unsqueeze(0)
    if v.dim() != 4 or v.shape[1] not in (1, 3) or v.dtype != torch.float32 or v.numel() == 0:
        raise RuntimeError("dihedral_variants expects fp32 pictures [N,C,H,W] with C = 1 or 3, got %s %s" % (x.dtype, tuple(x.shape)))
    n, c, h, w = (int(s) for s in v.shape)
    buf = torch.empty(8 * n * h * w * c, dtype=torch.float32, device=v.device)
    check(_lib.load().srk_dihedral_variants(ptr(v), int(v.stride(0)), int(v.stride(1)), int(v.stride(2)), int(v.stride(3)),
                                            n, c, h, w, ptr(buf), stream_ptr()), "srk_dihedral_variants")
    half = 4 * n * h * w * c
    even = buf[:half].view(4 * n, h, w, c).permute(0, 3, 1, 2)
    odd = buf[half:].view(4 * n, w, h, c).permute(0, 3, 1, 2)
    whole = buf.view(8 * n, h, w, c).permute(0, 3, 1, 2) if h == w else None
    return DihedralVariants(even, odd, whole)


def _merge_sources(what, even, odd):
    require_cuda(even, odd)
    e, o = even.detach(), odd.detach()
    if (e.dim() != 4 or o.dim() != 4 or e.dtype != torch.float32 or o.dtype != torch.float32 or e.shape[1] not in (1, 3)
            or e.shape[0] % 4 or e.numel() == 0
            or tuple(o.shape) != (e.shape[0], e.shape[1], e.shape[3], e.shape[2])):
        raise RuntimeError("%s expects fp32 net outputs even [4N,C,oh,ow] and odd [4N,C,ow,oh] with C = 1 or 3, got %s %s and "
                           "%s %s" % (what, even.dtype, tuple(even.shape), odd.dtype, tuple(odd.shape)))
    if o.device != e.device:
        raise RuntimeError("%s: even is on %s and odd on %s" % (what, e.device, o.device))
    return e, o, _strides4(e), _strides4(o)


def dihedral_merge(even, odd, out=None):
    """The ensemble E = (((((((y_0 + y_1) + y_2) + y_3) + y_4) + y_5) + y_6) + y_7) * 0.125, y_k = T_k^-1 of the net's
    output for variant k, in fp32 and in that order, in one launch: even [4N,C,oh,ow] (k = 0, 2, 4, 6 per picture) and odd
    [4N,C,ow,oh] (k = 1, 3, 5, 7) are read in place through their strides (NCHW or channels-last) -> [N,C,oh,ow]."""
    e, o, se, so = _merge_sources("dihedral_merge", even, odd)
    n, c, oh, ow = int(e.shape[0]) // 4, int(e.shape[1]), int(e.shape[2]), int(e.shape[3])
    out = _f32_out("dihedral_merge", (n, c, oh, ow), e.device, out)
    check(_lib.load().srk_dihedral_merge_f32(ptr(e), se, ptr(o), so, n, c, oh, ow, ptr(out), stream_ptr()),
          "srk_dihedral_merge_f32")
    return out


def dihedral_merge_u8(even, odd, cb=None, cr=None):
    """dihedral_merge of ONE picture writing the final 8-bit picture directly: to_u8_image(dihedral_merge(...)) without
    the fp32 mean (uint8 [oh,ow,C]), or with the chroma planes cb / cr (uint8 [oh,ow]; C = 1)
    ycbcr_to_rgb_u8(dihedral_merge(...), cb, cr) (uint8 [oh,ow,3]); bit-equal to those compositions."""
    e, o, se, so = _merge_sources("dihedral_merge_u8", even, odd)
    c, oh, ow = int(e.shape[1]), int(e.shape[2]), int(e.shape[3])
    if e.shape[0] != 4:
        raise RuntimeError("dihedral_merge_u8 writes one picture: even must be [4,C,oh,ow], got %s" % (tuple(even.shape),))
    cb, cr, out = _u8_out("dihedral_merge_u8", c, oh, ow, e.device, cb, cr)
    check(_lib.load().srk_dihedral_merge_u8(ptr(e), se, ptr(o), so, c, oh, ow, None if cb is None else ptr(cb),
                                            None if cr is None else ptr(cr), ptr(out), stream_ptr()), "srk_dihedral_merge_u8")
    return out


# ------------------------------------------------------------------------------------------------
# DRCN (drcn.py:13-59): the weight-shared recursion and the recursive-supervision head
# ------------------------------------------------------------------------------------------------
# The inference net applies ONE conv + ReLU D times in a row and ONE two-conv reconstruction to each of the D hidden
# states.  Built from ordinary conv calls that is D + 2D weight-gradient records writing the same three dw tensors, and
# pending_wgrad_groups() (no two records of a group writing one dw) would turn each into a launch group of its own.
# Instead the D hidden states live in ONE stacked NHWC buffer H[(D+1)*N] (H[0] = h0): the reconstruction runs as
# ordinary layers on the batch D*N (two launches and one weight-gradient record per conv), and the recursion's weight
# gradient is ONE record over the stacked batch (x = H[0:D], dy = the stacked gradient, mask = H[1:D+1]).
def _copy_amax_tag(src, dst):
    a = getattr(src, "_srk_amax", None)
    if a is not None and a[1] == _ver(src) and a[2] == _AMAX_EPOCH[0]:
        _tag_amax(dst, a[0])


def _recursion_forward(h0, weight, bias, D, cfg, packed, role):
    """H[(D+1)*N, F, H, W] with H[0] = h0 and H[d] = relu(conv(H[d-1])), one conv launch per slice.  Returns (H, the
    D+1 slice views): the views carry the running maxima the kernels leave, so every application takes the arithmetic
    a chain of separate conv calls would."""
    n, f, hh, ww = h0.shape
    H = _empty_cl((D + 1) * n, f, hh, ww, h0)
    sl = [H[d * n:(d + 1) * n] for d in range(D + 1)]
    sl[0].copy_(h0)
    _copy_amax_tag(h0, sl[0])
    if packed is not None:
        wp, bp = packed[0], packed[1]
    else:
        wp, bp = pack_weight_fwd(weight, False, 0), bias
    for d in range(1, D + 1):
        conv_forward_raw(sl[d - 1], wp, bp, weight, cfg, role=role, out=sl[d])
    return H, sl


class _Recursion(torch.autograd.Function):
    """H[1:] = the D applications of relu(conv(., weight, bias)) to h0, stacked along the batch axis."""

    @staticmethod
    def forward(ctx, h0, weight, bias, D, cfg, packed):
        h0 = to_nhwc(h0)
        H, sl = _recursion_forward(h0, weight, bias, D, cfg, packed, "train_fwd")
        ctx.sl, ctx.D, ctx.cfg = sl, D, cfg
        ctx.H = H
        ctx.weight_ref, ctx.bias_ref = weight, bias
        ctx.wpb = packed[2] if packed is not None and len(packed) > 2 else None
        ctx.save_for_backward(weight)
        return H[h0.shape[0]:]

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        (weight,) = ctx.saved_tensors
        D, sl, cfg, H = ctx.D, ctx.sl, ctx.cfg, ctx.H
        n = sl[0].shape[0]
        g = to_nhwc(g if (_is_nchw_dense(g) or _is_nhwc_dense(g)) else g.contiguous())
        gs = [g[d * n:(d + 1) * n] for d in range(D)]        # what the reconstruction sends to h_{d+1}
        U = _empty_cl(D * n, *g.shape[1:], g)                 # u_{d+1}: the whole gradient reaching h_{d+1}
        us = [U[d * n:(d + 1) * n] for d in range(D)]
        us[D - 1].copy_(gs[D - 1])
        d1 = _make_desc(sl[0].shape, weight, cfg, "bwd")
        wpb = ctx.wpb if ctx.wpb is not None else pack_weight_bwd(weight, False)
        # the data-gradient chain: u_{d+1} = conv^T(relu'(h_{d+2}) * u_{d+2}) + g_{d+1}, the add in the kernel's epilogue
        for i in range(D - 2, -1, -1):
            mask = BwdMask(ptr(sl[i + 2]), 0.0)
            check(lib.srk_conv2d_backward_data(ctypes.byref(d1), ptr(us[i + 1]), ptr(wpb), ptr(us[i]), ctypes.byref(mask),
                                               ptr(gs[i]), stream_ptr()), "srk_conv2d_backward_data")
        dh0 = None
        if ctx.needs_input_grad[0]:
            dh0 = _empty_cl(n, *g.shape[1:], g)
            mask = BwdMask(ptr(sl[1]), 0.0)
            check(lib.srk_conv2d_backward_data(ctypes.byref(d1), ptr(us[0]), ptr(wpb), ptr(dh0), ctypes.byref(mask), None,
                                               stream_ptr()), "srk_conv2d_backward_data")
        # ONE weight gradient over the stacked batch: x = H[0:D], dy = U, mask = relu'(H[1:D+1])
        xs, ys = H[:D * n], H[n:]
        dw, db = _weight_grad(_make_desc(xs.shape, weight, cfg, "bwd"), xs, U, ctx.weight_ref, ctx.bias_ref,
                              ctx.needs_input_grad[1] or (ctx.bias_ref is not None and ctx.needs_input_grad[2]), ys, 0.0)
        return dh0, dw, db, None, None, None


def recursive_conv(h0, weight, bias, D, cfg=None, packed=None):
    """drcn.py:41-44: h_{d+1} = relu(conv(h_d, weight, bias)) for d = 0..D-1 with ONE shared filter.  Returns the D
    hidden states h_1..h_D as one [D*N, F, H, W] channels_last tensor (h_d = rows (d-1)*N .. d*N-1).  cfg: the conv's
    stride / padding (default 1 / 1; the activation is always ReLU).  packed: (wp_fwd, bias[, wp_bwd]) of a PackPlan or
    a no-grad cache.  Under no_grad nothing is kept for a backward pass."""
    require_cuda(h0, weight, bias)
    if D < 1:
        raise ValueError("recursive_conv: D must be >= 1")
    cfg = ConvCfg(1 if cfg is None else cfg.stride, 1 if cfg is None else cfg.pad, act=ACT_RELU)
    cout, cin, _, _ = weight.shape
    if cout != cin or h0.shape[1] != cin:
        raise RuntimeError("recursive_conv: a recursion needs an F -> F filter and F-channel input (got %s, %s)"
                           % (tuple(weight.shape), tuple(h0.shape)))
    from .layers import grad_mode
    if grad_mode(h0, weight, bias):
        return _Recursion.apply(h0, weight, bias, int(D), cfg, packed)
    with torch.no_grad():
        H, sl = _recursion_forward(to_nhwc(h0), weight, bias, int(D), cfg, packed, "infer")
        return H[h0.shape[0]:]


class _DRCNHead(torch.autograd.Function):
    """(loss, out, terms) of srk_drcn_head_loss; the gradients to Y and w come from the forward pass (the seed contract
    of the losses, _declare_seed).  out and terms carry no gradient."""

    @staticmethod
    def forward(ctx, Y, x, w, target, alpha, reg, D, need_grad):
        lib = _lib.load()
        n = Y.shape[0] // D
        c, h, wd = Y.shape[1:]
        out = _empty_cl(n, c, h, wd, Y)
        dY = torch.empty_like(Y)
        loss = torch.empty((), dtype=torch.float32, device=Y.device)
        terms = torch.empty(2, dtype=torch.float32, device=Y.device)
        ws = torch.empty(max(int(lib.srk_drcn_workspace_bytes(D)), 16), dtype=torch.uint8, device=Y.device)
        wacc = getattr(w, "_srk_grad", None) if need_grad else None
        dw = None
        if need_grad:
            dw = wacc if wacc is not None else torch.empty_like(w)
        check(lib.srk_drcn_head_loss(ptr(Y), ptr(x), ptr(target), ptr(w), D, n, c, h, wd, ptr(alpha), ptr(reg),
                                     _declare_seed(ctx), ptr(out), ptr(dY), ptr(loss), ptr(terms), ptr(dw), 0.0, ptr(ws),
                                     ws.numel(), stream_ptr()), "srk_drcn_head_loss")
        ctx.grads = (dY, dw) if need_grad else (None, None)
        ctx.w_in_place = wacc is not None
        ctx.mark_non_differentiable(out, terms)
        return loss, out, terms

    @staticmethod
    def backward(ctx, g, g_out, g_terms):
        dY, dw = _seed_scaled(ctx, g, ctx.grads)
        if ctx.w_in_place:      # w's gradient lives in its _srk_grad view: a scaled one goes back there, none is returned
            if dw is not ctx.grads[1]:
                ctx.grads[1].copy_(dw)
            dw = None
        return dY, None, dw, None, None, None, None, None


def _drcn_combine_raw(Y, x, w, D):
    lib = _lib.load()
    n = Y.shape[0] // D
    c, h, wd = Y.shape[1:]
    out = _empty_cl(n, c, h, wd, Y)
    check(lib.srk_drcn_head_forward(ptr(Y), ptr(x), ptr(w), D, n, c, h, wd, ptr(out), stream_ptr()),
          "srk_drcn_head_forward")
    return out


class _DRCNCombine(torch.autograd.Function):
    """out = x + sum_d w_d Y_d / sum w with its gradients (srk_drcn_head_backward): the head without a target, for a
    loss the caller composes itself (the reference's own loop, drcn.py:203-215, differentiates `out` directly)."""

    @staticmethod
    def forward(ctx, Y, x, w, D):
        ctx.D = D
        ctx.save_for_backward(Y, w)
        return _drcn_combine_raw(Y, x, w, D)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        Y, w = ctx.saved_tensors
        D = ctx.D
        n = Y.shape[0] // D
        c, h, wd = Y.shape[1:]
        g = to_nhwc(g if (_is_nchw_dense(g) or _is_nhwc_dense(g)) else g.contiguous())
        dY = torch.empty_like(Y)
        dw = torch.empty_like(w) if ctx.needs_input_grad[2] else None
        ws = torch.empty(max(int(lib.srk_drcn_workspace_bytes(D)), 16), dtype=torch.uint8, device=Y.device)
        check(lib.srk_drcn_head_backward(ptr(Y), ptr(w), ptr(g), D, n, c, h, wd, ptr(dY), ptr(dw), 0.0, ptr(ws),
                                         ws.numel(), stream_ptr()), "srk_drcn_head_backward")
        return (dY if ctx.needs_input_grad[0] else None), (g if ctx.needs_input_grad[1] else None), dw, None


def _scalar_dev(t, what, like):
    if t is None:
        return
    if t.numel() != 1 or t.dtype != torch.float32 or t.device != like.device:
        raise RuntimeError("drcn_head: %s must be a one-element float32 tensor on %s (got %s %s on %s)"
                           % (what, like.device, tuple(t.shape), t.dtype, t.device))


def drcn_head(Y, x, w, target=None, alpha=None, reg=None, parts=False):
    """drcn.py:46-52 and 203-215.  Y: the D reconstructions stacked along the batch axis ([D*N, C, H, W], as the
    reconstruction layer produces them from recursive_conv's output); x: the net input; w: the D combine weights.
      target None: out = x + sum_d w_d Y_d / sum w, differentiable in Y, x and w when autograd records (the
      inference combine otherwise).
      else: the scalar loss alpha * mean_d MSE(Y_d, t) + (1 - alpha) * MSE(out, t) + reg, with its gradient to Y and w
      computed in the same pass.  alpha / reg: 0-dim device tensors (read by the kernel: a captured step stays valid
      when they change); reg = the weight-decay value beta * R (sumsq), None = 0.  A w with a `_srk_grad` view (the
      trainer's optimizer) gets its gradient written there directly.  parts=True returns (loss, out, [L1, L2])."""
    D = int(w.numel())
    require_cuda(Y, x, w, target, alpha, reg)
    if Y.dim() != 4 or Y.shape[0] % D:
        raise RuntimeError("drcn_head: Y must be [D*N, C, H, W] with D = %d (got %s)" % (D, tuple(Y.shape)))
    n = Y.shape[0] // D
    if tuple(x.shape) != (n,) + tuple(Y.shape[1:]):
        raise RuntimeError("drcn_head: x %s does not match one reconstruction %s" % (tuple(x.shape), (n,) + tuple(Y.shape[1:])))
    if w.dtype != torch.float32 or w.device != Y.device:
        raise RuntimeError("drcn_head: w must be float32 on %s (got %s on %s)" % (Y.device, w.dtype, w.device))
    Y, x = to_nhwc(Y), to_nhwc(x)
    w = w if w.is_contiguous() else w.contiguous()
    from .layers import grad_mode
    if target is None:
        if grad_mode(Y, x, w):
            return _DRCNCombine.apply(Y, x, w, D)
        return _drcn_combine_raw(Y, x, w.detach(), D)
    if tuple(target.shape) != tuple(x.shape):
        raise RuntimeError("drcn_head: target %s vs output %s" % (tuple(target.shape), tuple(x.shape)))
    if alpha is None:
        raise RuntimeError("drcn_head: a target needs alpha (a one-element float32 device tensor)")
    _scalar_dev(alpha, "alpha", Y)
    _scalar_dev(reg, "reg", Y)
    loss, out, terms = _DRCNHead.apply(Y, x.detach(), w, to_nhwc(target).detach(), alpha, reg, D, grad_mode(Y, w))
    return (loss, out, terms) if parts else loss


def sumsq(p, scale=1.0, out=None):
    """scale * sum(p^2) of a dense fp32 tensor (a FlatParams data buffer: the weight-decay value of drcn.py:212-214) as a
    0-dim device tensor, accumulated in fp64.  out: a 0-dim tensor to write instead of a new one."""
    require_cuda(p)
    p = p.detach()
    if not p.is_contiguous():
        raise RuntimeError("sumsq: p must be contiguous")
    lib = _lib.load()
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=p.device)
    elif out.numel() != 1 or out.dtype != torch.float32 or out.device != p.device:
        raise RuntimeError("sumsq: out must be a one-element float32 tensor on %s (got %s %s on %s)"
                           % (p.device, tuple(out.shape), out.dtype, out.device))
    ws = torch.empty(int(lib.srk_sumsq_workspace_bytes()), dtype=torch.uint8, device=p.device)
    check(lib.srk_sumsq(ptr(p), p.numel(), float(scale), ptr(out), ptr(ws), stream_ptr()), "srk_sumsq")
    return out


def add_scaled_(a, b, beta):
    """a += beta * b in place (srk_axpby; flat buffers: DRCN's weight-decay gradient 2 * beta * theta)."""
    lib = _lib.load()
    check(lib.srk_axpby(ptr(a), ptr(b), ptr(a), a.numel(), 1.0, float(beta), stream_ptr()), "srk_axpby")
    return a


# ------------------------------------------------------------------------------------------------
# Channel attention (RCAN's gate; csrc/ca.hip)
# ------------------------------------------------------------------------------------------------
def _ca_workspace(lib, t):
    n, c, h, w = t.shape
    nbytes = int(lib.srk_channel_attention_workspace(n, h, w, c))
    return torch.empty(max(nbytes, 8), dtype=torch.uint8, device=t.device), nbytes   # torch's allocator: a graph owns it


class _ChannelAttention(torch.autograd.Function):
    """y = t * sigmoid(W2 relu(W1 mean_hw(t) + b1) + b2) (+ x): two launches forward, three backward; saves t, m, h, s."""

    @staticmethod
    def forward(ctx, t, x, w1, b1, w2, b2, res_box=None):
        lib = _lib.load()
        require_cuda(t, x, w1, b1, w2, b2)
        if t.dim() != 4:
            raise RuntimeError("channel_attention: expected a 4-D NCHW tensor, got shape %s" % (tuple(t.shape),))
        n, c, hh, ww = t.shape
        cr = w1.shape[0]
        if tuple(w1.shape[:2]) != (cr, c) or w1.numel() != cr * c or tuple(w2.shape[:2]) != (c, cr) \
                or w2.numel() != c * cr or b1.numel() != cr or b2.numel() != c:
            raise RuntimeError("channel_attention: weights %s, %s and biases %s, %s do not fit C = %d"
                               % (tuple(w1.shape), tuple(w2.shape), tuple(b1.shape), tuple(b2.shape), c))
        if x is not None and x.shape != t.shape:
            raise RuntimeError("channel_attention: skip %s vs input %s" % (tuple(x.shape), tuple(t.shape)))
        t = _dense(t)
        x = _dense(x) if x is not None else None
        w1c, b1c, w2c, b2c = (p.detach().contiguous() for p in (w1, b1, w2, b2))
        need_grad = any(ctx.needs_input_grad)
        y = torch.empty_like(t)
        m = h = s = None
        if need_grad:
            m = torch.empty((n, c), dtype=torch.float32, device=t.device)
            h = torch.empty((n, cr), dtype=torch.float32, device=t.device)
            s = torch.empty((n, c), dtype=torch.float32, device=t.device)
        ws, nbytes = _ca_workspace(lib, t)
        check(lib.srk_channel_attention_forward(ptr(t), ptr(x), ptr(w1c), ptr(b1c), ptr(w2c), ptr(b2c), n, hh, ww, c, cr,
                                                ptr(y), ptr(m), ptr(h), ptr(s), ptr(ws), nbytes, stream_ptr()),
              "srk_channel_attention_forward")
        ctx.has_skip, ctx.res_box = x is not None, res_box
        ctx.params = (w1, b1, w2, b2)
        if need_grad:
            ctx.save_for_backward(t, m, h, s, w1c, w2c)
        return y

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        t, m, h, s, w1c, w2c = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        n, c, hh, ww = t.shape
        cr = h.shape[1]
        g = _dense(g)
        dt = torch.empty_like(t)
        need = ctx.needs_input_grad[2:6]
        acc = [getattr(p, "_srk_grad", None) for p in (w1, b1, w2, b2)]
        flat = all(a is not None for a in acc)     # optim.FlatParams: accumulate into the flat gradient buffer
        if flat:
            outs, beta = [a if nd else None for a, nd in zip(acc, need)], 1.0
        else:
            outs, beta = [torch.empty(p.shape, dtype=torch.float32, device=t.device) if nd else None
                          for p, nd in zip((w1, b1, w2, b2), need)], 0.0
        ws, nbytes = _ca_workspace(lib, t)
        check(lib.srk_channel_attention_backward(ptr(g), ptr(t), ptr(w1c), ptr(w2c), ptr(m), ptr(h), ptr(s), n, hh, ww, c,
                                                 cr, ptr(dt), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), beta,
                                                 ptr(ws), nbytes, stream_ptr()), "srk_channel_attention_backward")
        dx = g if ctx.has_skip else None      # the skip's gradient is g itself: no kernel
        if dx is not None and ctx.res_box is not None:
            ctx.res_box.g, dx = dx, None      # consumed by the block's first conv (GradBox)
        if flat:
            outs = [None] * 4
        return (dt if ctx.needs_input_grad[0] else None, dx) + tuple(outs) + (None,)


def channel_attention(t, x, w1, b1, w2, b2, res_box=None):
    """Channel attention with the skip add fused: y = t * s (+ x), s = sigmoid(W2 relu(W1 m + b1) + b2), m the mean of t
    over each sample's pixels.  t, x: [N,C,H,W], NCHW-contiguous or channels_last (x may be None); w1 [Cr,C] or
    [Cr,C,1,1], w2 [C,Cr] or [C,Cr,1,1] (1x1 conv filters), b1 [Cr], b2 [C].  The gradient of x is the gradient of y
    itself; res_box: the ops.GradBox that takes it instead (base_networks.RCAB).  include/srk.h:
    srk_channel_attention_forward / _backward."""
    return _ChannelAttention.apply(t, x, w1, b1, w2, b2, res_box)


# ------------------------------------------------------------------------------------------------
# LPIPS (Zhang et al. 2018, the VGG variant; csrc/lpips.hip)
# ------------------------------------------------------------------------------------------------
def _nhwc(x):
    return to_nhwc(x if (_is_nchw_dense(x) or _is_nhwc_dense(x)) else x.contiguous())


class _LpipsLayer(torch.autograd.Function):
    """One tapped layer's distance: writes table[row][n] = mean_hw sum_c w[c] (f0[c] / a - f1[c] / b)^2 (two launches)
    and returns that row; the backward (one launch) recomputes the norms from the two saved maps.  Gradient: f_pred only."""

    @staticmethod
    def forward(ctx, f_pred, f_target, w, row, table):
        lib = _lib.load()
        require_cuda(f_pred, f_target, w)
        if f_pred.dim() != 4 or f_pred.shape != f_target.shape:
            raise RuntimeError("lpips_layer: feature maps %s and %s must be equal 4-D NCHW shapes"
                               % (tuple(f_pred.shape), tuple(f_target.shape)))
        n, c, h, ww = f_pred.shape
        if w.numel() != c:
            raise RuntimeError("lpips_layer: %d weights for %d channels" % (w.numel(), c))
        if (table.dtype != torch.float64 or not table.is_cuda or table.dim() != 2 or table.shape[1] != n
                or not table.is_contiguous()):
            raise RuntimeError("lpips_layer: table must be a contiguous float64 [L, %d] device tensor, got %s %s"
                               % (n, table.dtype, tuple(table.shape)))
        row = int(row)
        if not 0 <= row < table.shape[0]:
            raise RuntimeError("lpips_layer: row %d of a table of %d rows" % (row, table.shape[0]))
        f0 = _nhwc(f_pred)
        f1 = f0 if f_target is f_pred else _nhwc(f_target.detach())
        wc = w.detach().reshape(-1).contiguous()
        nbytes = int(lib.srk_lpips_layer_workspace(n, h, ww, c))
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=f0.device)   # torch's allocator: a graph owns it
        check(lib.srk_lpips_layer_forward(ptr(f0), ptr(f1), ptr(wc), n, h, ww, c, row, table.shape[0], ptr(table), ptr(ws),
                                          nbytes, stream_ptr()), "srk_lpips_layer_forward")
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(f0, f1, wc)
        return table[row]

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        f0, f1, wc = ctx.saved_tensors
        n, c, h, ww = f0.shape
        g = g.to(torch.float64).contiguous()   # (what _LpipsFinish hands out already is both)
        df0 = _empty_cl(n, c, h, ww, f0)
        check(lib.srk_lpips_layer_backward(ptr(f0), ptr(f1), ptr(wc), ptr(g), n, h, ww, c, ptr(df0), stream_ptr()),
              "srk_lpips_layer_backward")
        return df0, None, None, None, None


def lpips_layer(f_pred, f_target, w, row, table):
    """The LPIPS distance of one tapped layer, fused: per pixel both maps are normalised over their channels, subtracted,
    squared and weighed by w [C], and the mean over the sample's pixels goes to table[row] (`table`: float64 [L, N] on the
    device, written in place by the kernels; the returned [N] tensor is that row, a view -- nothing else may write the
    table in place before the backward has run).  f_pred, f_target: [N,C,H,W], NCHW-contiguous or
    channels_last.  The gradient goes to f_pred only: d(row[n]) / d f_pred times the [N] float64 gradient of the row.
    include/srk.h: srk_lpips_layer_forward / _backward."""
    return _LpipsLayer.apply(f_pred, f_target, w, row, table)


class _LpipsFinish(torch.autograd.Function):
    """The L rows of the table added in order (one launch): the per-sample values [N], or their mean under the seed contract
    of the losses (_declare_seed) -- the same launch writes seed / N for every sample, the
    gradient of each row, so a backward seeded as declared runs no arithmetic of its own.  `rows`: what lpips_layer
    returned, one per row (they tie the layers into the graph)."""

    @staticmethod
    def forward(ctx, table, reduce, *rows):
        lib = _lib.load()
        nl, n = table.shape
        need = any(ctx.needs_input_grad[2:])
        out = torch.empty(n if not reduce else (), dtype=torch.float32, device=table.device)
        gvec = torch.empty(n, dtype=torch.float64, device=table.device) if (need and reduce) else None
        check(lib.srk_lpips_finish(ptr(table), nl, n, _declare_seed(ctx, reduce), None if reduce else ptr(out),
                                   ptr(out) if reduce else None, ptr(gvec), stream_ptr()), "srk_lpips_finish")
        ctx.reduce, ctx.gvec, ctx.k, ctx.need = reduce, gvec, len(rows), need
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.need:
            return (None,) * (2 + ctx.k)
        if not ctx.reduce:
            gv = g.to(torch.float64).contiguous()       # the per-sample gradients as they come
        elif _is_own_seed(ctx, g, g.device):            # the seed this loss was computed for: already in gvec
            gv = ctx.gvec
        else:                                           # some other upstream gradient: gvec = seed / N, a fp64 row
            gv = ctx.gvec * (g.to(torch.float64) / ctx.seed_value)
        return (None, None) + (gv,) * ctx.k


LPIPS_SHIFT, LPIPS_SCALE = (-.030, -.088, -.188), (.458, .448, .450)


def lpips_input_affine(normalize=True):
    """(sub, div) of the one channel_affine call in front of the LPIPS net: (x - shift) / scale on inputs in [-1, 1], or
    with `normalize` ((2 x - 1) - shift) / scale = (x - (1 + shift) / 2) / (scale / 2) on inputs in [0, 1]."""
    if normalize:
        return tuple((1.0 + s) / 2.0 for s in LPIPS_SHIFT), tuple(s / 2.0 for s in LPIPS_SCALE)
    return LPIPS_SHIFT, LPIPS_SCALE


def lpips(pred, target, net, normalize=True, reduce=True):
    """LPIPS (Zhang et al. 2018, the VGG variant) of pred against target: the five tapped VGG16 maps of both, each pair
    through lpips_layer, the five values added.  reduce=True: the mean over the batch as a 0-dim fp32 device tensor with
    the seed contract of the losses (_declare_seed); reduce=False: the per-sample
    values [N].  normalize: the inputs are in [0, 1] (True) or already in [-1, 1] (False).  The gradient flows to pred
    only; both operands run the same kernels (the target's without a graph), so equal inputs give exactly 0 and a zero
    gradient.  pred / target: [N, 3, H, W] on the device with H, W >= 16; net: models.LPIPS."""
    for name, t in (("pred", pred), ("target", target)):
        if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 3:
            raise ValueError("lpips: %s must be [N, 3, H, W] (LPIPS reads RGB), got shape %s"
                             % (name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    if pred.shape != target.shape:
        raise ValueError("lpips: pred %s vs target %s" % (tuple(pred.shape), tuple(target.shape)))
    if min(pred.shape[2:]) < 16:
        raise ValueError("lpips: pictures of %d x %d, the five taps need at least 16 on a side" % tuple(pred.shape[2:]))
    if not (pred.is_cuda and target.is_cuda):
        raise ValueError("lpips: pred (%s) and target (%s) must be on the device" % (pred.device, target.device))
    sub, div = lpips_input_affine(normalize)
    with torch.no_grad():
        real = net.extract(channel_affine(target.detach(), sub, div), grad=True)
    fake = net.extract(channel_affine(pred, sub, div), grad=True)
    table = torch.empty((len(fake), pred.shape[0]), dtype=torch.float64, device=pred.device)
    rows = [lpips_layer(a, b, w, l, table) for l, (a, b, w) in enumerate(zip(fake, real, net.lins))]
    return _LpipsFinish.apply(table, bool(reduce), *rows)


# ------------------------------------------------------------------------------------------------
# Convolution over channel slices and the residual-dense trunk of RDN (csrc/dense.hip)
# ------------------------------------------------------------------------------------------------
def dense_terms(role):
    """MFMA products per multiplication of the slice convolutions in the current precision mode: 3 where _MODES asks for
    ALGO_AUTO (the bf16x3 class), 6 for the fp32-faithful class -- and for 'fp32', whose exact-fp32 MFMA kernel the
    six-term split is tighter than (see _MODES).  role: 'infer' | 'train_fwd' | 'bwd'."""
    return 3 if _MODES[_PRECISION["mode"]][role] in (ALGO_AUTO, _lib.ALGO_MFMA_BF16X3) else 6


def _dense_check(rc, what):
    """check(), but a request no kernel covers is the caller's ValueError (the message names the number): there is no
    concatenating fallback."""
    if rc == _lib.ERR_UNSUPPORTED:
        raise ValueError("%s: %s" % (what, _lib.load().srk_last_error_string().decode()))
    check(rc, what)


def _dense_launch(name, args, e=None, at=None):
    """srk_dense_conv_<name>(*args), or with a DenseEpilogue `e` its _ex twin, which takes `e` as argument number `at`:
    the one place that chooses between the two (they are different kernel instantiations)."""
    symbol = "srk_dense_conv_" + name
    if e is not None:
        symbol += "_ex"
        args.insert(at, ctypes.byref(e))
    _dense_check(getattr(_lib.load(), symbol)(*args), symbol)


class _Slice(object):
    """`channels` channels of a dense NHWC buffer, from channel `off`: pointer and pixel stride for the kernels."""
    __slots__ = ("t", "off", "channels", "ld", "p")

    def __init__(self, what, t, off, channels, like=None):
        if not torch.is_tensor(t) or t.dim() != 4 or not t.is_cuda or t.dtype != torch.float32 or not _is_nhwc_dense(t):
            raise RuntimeError("%s: a channels_last fp32 [N, C, H, W] tensor on the device is expected, got %s"
                               % (what, (tuple(t.shape), t.stride(), t.dtype, t.device) if torch.is_tensor(t) else type(t)))
        off, channels = int(off), int(channels)
        if off < 0 or channels < 0 or off + channels > t.shape[1]:
            raise ValueError("%s: channels [%d, %d) do not lie in the buffer's %d" % (what, off, off + channels, t.shape[1]))
        if like is not None and (t.shape[0], t.shape[2], t.shape[3]) != (like.t.shape[0], like.t.shape[2], like.t.shape[3]):
            raise ValueError("%s: %s vs %s: batch and picture sizes differ" % (what, tuple(t.shape), tuple(like.t.shape)))
        self.t, self.off, self.channels, self.ld = t, off, channels, int(t.shape[1])
        self.p = ctypes.c_void_p(t.data_ptr() + 4 * off)


_NO_SLICE = _Slice.__new__(_Slice)      # an operand the call does not have: a null pointer, no channels, stride 0
_NO_SLICE.t, _NO_SLICE.off, _NO_SLICE.channels, _NO_SLICE.ld, _NO_SLICE.p = None, 0, 0, 0, None


def _dense_inputs(what, a, a_off, ca, b, b_off, cb):
    """The slices (a, b) a convolution or its weight gradient reads; no b without a buffer or with cb = 0."""
    sa = _Slice(what + ": a", a, a_off, a.shape[1] - a_off if ca is None else ca)
    if b is not None and (cb is None or cb > 0):
        return sa, _Slice(what + ": b", b, b_off, b.shape[1] - b_off if cb is None else cb, sa)
    return sa, _NO_SLICE


def _dense_desc(what, like, weight, ca, cb, act, slope, terms):
    """The descriptor of a convolution with `weight` (or its gradient) [Cout, ca + cb, K, K] over pictures the size of the
    slice `like`'s, every stride still 0: the caller fills in those of the operands it has."""
    d = _lib.DenseDesc()
    d.N, d.H, d.W = int(like.t.shape[0]), int(like.t.shape[2]), int(like.t.shape[3])
    d.K, d.CA, d.CB, d.Cout = int(weight.shape[2]), int(ca), int(cb), int(weight.shape[0])
    d.act, d.slope, d.terms = int(act), float(slope), int(terms)
    if tuple(weight.shape) != (d.Cout, d.CA + d.CB, d.K, d.K) or not weight.is_contiguous():
        raise ValueError("%s: a contiguous weight [%d, %d, %d, %d] is expected, got %s"
                         % (what, d.Cout, d.CA + d.CB, d.K, d.K, tuple(weight.shape)))
    return d


def dense_conv(a, weight, bias=None, b=None, out=None, ca=None, a_off=0, cb=None, b_off=0, out_off=0, act=ACT_NONE,
               slope=0.0, residual=None, res_off=0, terms=3, s=None, r1=1.0, residual2=None, res2_off=0, r2=1.0):
    """out[:, out_off : out_off + Cout] = act(conv(cat(a[:, a_off : a_off + ca], b[:, b_off : b_off + cb]), weight) + bias)
    (+ residual[:, res_off : res_off + Cout]) without the cat: stride 1, 'same', K in {1, 3}.  a, b, out, residual:
    channels_last buffers of any width; no other channel of `out` is touched.  out=None: a new [N, Cout, H, W] tensor.
    No autograd (ops.residual_dense_blocks is the differentiable user).  ValueError for what no kernel covers.
    With `s` (or residual2) the call is srk_dense_conv_forward_ex:
    out = s * act(conv + bias) + r1 * residual + r2 * residual2[:, res2_off : res2_off + Cout] (s=None: 1)."""
    what = "dense_conv"
    cout = int(weight.shape[0])
    sa, sb = _dense_inputs(what, a, a_off, ca, b, b_off, cb)
    if out is None:
        out = _empty_cl(a.shape[0], cout, a.shape[2], a.shape[3], a)
    so = _Slice(what + ": out", out, out_off, cout, sa)
    d = _dense_desc(what, sa, weight, sa.channels, sb.channels, act, slope, terms)
    sr = _Slice(what + ": residual", residual, res_off, cout, sa) if residual is not None else _NO_SLICE
    d.ldA, d.ldB, d.ldY, d.ldR = sa.ld, sb.ld, so.ld, sr.ld
    args = [ctypes.byref(d), sa.p, sb.p, ptr(weight), ptr(bias), sr.p, so.p, stream_ptr()]   # (an address needs no detach)
    e = None
    if s is not None or residual2 is not None:
        sr2 = _Slice(what + ": residual2", residual2, res2_off, cout, sa) if residual2 is not None else _NO_SLICE
        e = _lib.DenseEpilogue(1.0 if s is None else s, r1, r2, sr2.ld)
        args.insert(6, sr2.p)       # the _ex twin takes R2 behind R1, in front of its epilogue
    _dense_launch("forward", args, e, 7)
    return out


def dense_conv_backward_data(dy, weight, ca, cb=0, y_saved=None, da=None, db=None, add=None, dy_off=0, y_off=0, da_off=0,
                             db_off=0, add_off=0, beta_a=0.0, beta_b=0.0, act=ACT_NONE, slope=0.0, terms=3, s=None, a1=1.0):
    """The data gradient of dense_conv into the slices da[:, da_off : da_off + ca] and db[:, db_off : db_off + cb]
    (either may be None): slice = beta * slice + conv^T(dy * act'(y_saved)) (+ add into da), beta 0 or 1.  With `s` the
    call is srk_dense_conv_backward_data_ex: dy is scaled by s and add by a1."""
    what = "dense_conv_backward_data"
    cout = int(weight.shape[0])
    sdy = _Slice(what + ": dy", dy, dy_off, cout)
    d = _dense_desc(what, sdy, weight, ca, cb, act, slope, terms)
    sy = _Slice(what + ": y_saved", y_saved, y_off, cout, sdy) if y_saved is not None else _NO_SLICE
    sda = _Slice(what + ": da", da, da_off, ca, sdy) if da is not None else _NO_SLICE
    sdb = _Slice(what + ": db", db, db_off, cb, sdy) if db is not None and cb > 0 else _NO_SLICE
    sadd = _Slice(what + ": add", add, add_off, ca, sdy) if add is not None else _NO_SLICE
    d.ldDy, d.ldY, d.ldDA, d.ldDB, d.ldAdd = sdy.ld, sy.ld, sda.ld, sdb.ld, sadd.ld
    _dense_launch("backward_data", [ctypes.byref(d), sdy.p, sy.p, ptr(weight), sda.p, float(beta_a), sdb.p, float(beta_b),
                                    sadd.p, stream_ptr()], None if s is None else _lib.DenseEpilogue(s, a1=a1), 9)
    return da, db


def dense_conv_backward_weight(a, dy, dw, dbias=None, b=None, y_saved=None, ca=None, a_off=0, cb=None, b_off=0, dy_off=0,
                               y_off=0, beta=0.0, act=ACT_NONE, slope=0.0, terms=3, s=None):
    """dw = beta * dw + sum over pixels of cat(a, b)^T (dy * act'(y_saved)), dbias likewise (beta 0 or 1); dw is a
    contiguous [Cout, ca + cb, K, K] tensor or view (a parameter's slice of the flat gradient buffer).  Two launches, the
    pixel ranges added in a fixed order: two calls give the same bits.  With `s` the call is
    srk_dense_conv_backward_weight_ex: dy is scaled by s where the kernel reads it (no further launch)."""
    lib = _lib.load()
    what = "dense_conv_backward_weight"
    cout = int(dw.shape[0])
    sa, sb = _dense_inputs(what, a, a_off, ca, b, b_off, cb)
    sdy = _Slice(what + ": dy", dy, dy_off, cout, sa)
    d = _dense_desc(what, sa, dw, sa.channels, sb.channels, act, slope, terms)
    sy = _Slice(what + ": y_saved", y_saved, y_off, cout, sa) if y_saved is not None else _NO_SLICE
    d.ldA, d.ldB, d.ldDy, d.ldY = sa.ld, sb.ld, sdy.ld, sy.ld
    if lib.srk_dense_conv_plan(ctypes.byref(d), ctypes.byref(_lib.DensePlan())) == _lib.ERR_UNSUPPORTED:
        raise ValueError("%s: %s" % (what, lib.srk_last_error_string().decode()))
    nbytes = int(lib.srk_dense_conv_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=a.device)   # torch's allocator: a captured graph owns it
    _dense_launch("backward_weight", [ctypes.byref(d), sa.p, sb.p, sdy.p, sy.p, ptr(dw), ptr(dbias), float(beta), ptr(ws),
                                      nbytes, stream_ptr()], None if s is None else _lib.DenseEpilogue(s), 8)
    return dw, dbias


def _growth_buffer(n, c, h, w, like):
    """A block's growth buffer (its own name, so that a test can count them: one per call without a backward)."""
    return _empty_cl(n, c, h, w, like)


# One block core, two buffer policies: both trunks below (RDN here, ESRGAN in DESIGN.md 30) call it, and keep only where
# a block's input, output and gradients live and which skips its fusion convolution carries.
def _dense_block_forward(*, a, a_off, ca, layers, growth, out, out_off, act, slope, terms, s=None, r1=1.0, residual2=None,
                         r2=1.0):
    """layers = (w_1, b_1, .., w_C, b_C, w_fusion, b_fusion).  Growth convolution c reads the input a[:, a_off : a_off + ca]
    and growth[:, : (c - 1) G], and writes act(.) into growth[:, (c - 1) G : c G]; the fusion convolution reads
    [input | growth] and writes out[:, out_off : out_off + Cout] with the skip in its epilogue: conv + input, or with `s`
    (the _ex kernel) s * conv + r1 * input + r2 * residual2.  C + 1 launches."""
    C = len(layers) // 2 - 1
    g = int(layers[0].shape[0])
    for c in range(C):
        dense_conv(a, layers[2 * c], layers[2 * c + 1], b=growth if c else None, out=growth, ca=ca, a_off=a_off, cb=c * g,
                   out_off=c * g, act=act, slope=slope, terms=terms)
    dense_conv(a, layers[2 * C], layers[2 * C + 1], b=growth, out=out, ca=ca, a_off=a_off, cb=C * g, out_off=out_off,
               act=ACT_NONE, slope=0.0, residual=a, res_off=a_off, terms=terms, s=s, r1=r1, residual2=residual2, r2=r2)


def _dense_wgrad(layers, need, grads, i, a, dy, **conv):
    """dense_conv_backward_weight(a, dy, .., **conv) for layers[i], layers[i + 1] unless neither needs a gradient: added
    (beta 1) to their flat gradient buffer (optim.FlatParams), else written (beta 0) to a new dw, dbias kept in `grads`."""
    if not (need[i] or need[i + 1]):
        return
    acc = _flat_grads(layers[i], layers[i + 1])
    if acc is not None:
        dw, dbias, beta = acc[0], acc[1], 1.0
    else:
        dw = torch.empty_like(layers[i], memory_format=torch.contiguous_format)
        dbias, beta = torch.empty_like(layers[i + 1]), 0.0
        grads[i], grads[i + 1] = dw, dbias
    dense_conv_backward_weight(a, dy, dw, dbias=dbias, beta=beta, **conv)


def _dense_block_backward(*, a, a_off, ca, layers, need, growth, gg, dy, dy_off, da, da_off, beta_a, act, slope, terms,
                          s=None, a1=1.0, extra=None):
    """The backward of _dense_block_forward for the output gradient dy[:, dy_off : dy_off + Cout]; gg: room for the growth
    gradient.  The fusion convolution's data gradient starts gg (beta 0) and leaves beta_a * da + its share + the skip's
    gradient (dy itself; a1 * dy with `s`) in da[:, da_off : da_off + ca] in one epilogue; the growth convolutions C .. 1
    add theirs (beta 1), `extra`, one more gradient of the input, riding in the epilogue of the C-th.  da = None: nobody
    needs the input's gradient, one launch fewer.  Returns the parameter gradients autograd is to have (see _dense_wgrad)."""
    C = len(layers) // 2 - 1
    g = int(layers[0].shape[0])
    grads = [None] * len(layers)
    conv = dict(ca=ca, cb=C * g, dy_off=dy_off, terms=terms, s=s)
    _dense_wgrad(layers, need, grads, 2 * C, a, dy, b=growth, a_off=a_off, **conv)
    dense_conv_backward_data(dy, layers[2 * C], da=da, db=gg, add=dy if da is not None else None, da_off=da_off,
                             add_off=dy_off, beta_a=beta_a, beta_b=0.0, a1=a1, **conv)
    for c in reversed(range(C)):
        conv = dict(ca=ca, cb=c * g, y_saved=growth, dy_off=c * g, y_off=c * g, act=act, slope=slope, terms=terms)
        _dense_wgrad(layers, need, grads, 2 * c, a, gg, b=growth if c else None, a_off=a_off, **conv)
        if da is not None or c:
            dense_conv_backward_data(gg, layers[2 * c], da=da, db=gg if c else None, da_off=da_off, beta_a=1.0, beta_b=1.0,
                                     add=extra if (c == C - 1 and da is not None) else None, **conv)
    return grads


class _ResidualDenseBlocks(torch.autograd.Function):
    """D residual dense blocks on slice convolutions; see residual_dense_blocks."""

    @staticmethod
    def forward(ctx, x, D, C, need_grad, *params):
        require_cuda(x, *params)
        x = to_nhwc(x)
        n, g0, hh, ww = x.shape
        per = 2 * (C + 1)
        g = int(params[0].shape[0])
        # need_grad: decided by the caller, where the grad mode is still visible (needs_input_grad mirrors requires_grad
        # under torch.no_grad() too, and test() runs the training model there)
        terms = dense_terms("train_fwd" if need_grad else "infer")
        fusion = _empty_cl(n, D * g0, hh, ww, x)
        growths, growth = [], None
        for blk in range(D):
            if need_grad or growth is None:     # a backward reads every block's growth buffer: they are its ReLU masks
                growth = _growth_buffer(n, C * g, hh, ww, x)
            growths.append(growth)
            a, a_off = (x, 0) if blk == 0 else (fusion, (blk - 1) * g0)
            # the 1x1 local fusion adds the block's input and writes slice blk of the fusion buffer, the next block's input
            _dense_block_forward(a=a, a_off=a_off, ca=g0, layers=params[blk * per:(blk + 1) * per], growth=growth, out=fusion,
                                 out_off=blk * g0, act=ACT_RELU, slope=0.0, terms=terms)
        ctx.dims = (D, C, g0, g)
        ctx.params = params
        if need_grad:
            ctx.save_for_backward(x, fusion, *growths)
        return fusion

    @staticmethod
    def backward(ctx, gout):
        D, C, g0, g = ctx.dims
        params = ctx.params
        saved = ctx.saved_tensors
        x, fusion, growths = saved[0], saved[1], saved[2:]
        n, _, hh, ww = x.shape
        per = 2 * (C + 1)
        terms = dense_terms("bwd")
        gf = _dense(gout)                  # the fan-in accumulator: one copy, because autograd owns gout
        if gf is gout:                     # (a layout conversion already made one)
            gf = gout.clone(memory_format=torch.preserve_format)
        gg = _empty_cl(n, C * g, hh, ww, x)
        dx = _empty_cl(n, g0, hh, ww, x) if ctx.needs_input_grad[0] else None
        need, grads = ctx.needs_input_grad[4:], []
        for blk in reversed(range(D)):
            i0 = blk * per
            a, a_off = (x, 0) if blk == 0 else (fusion, (blk - 1) * g0)
            # block blk's output gradient is slice blk of gf; its input's gradient is accumulated (beta 1) into slice
            # blk - 1, where the blocks behind have already left theirs, and block 0 writes the dense dx (beta 0)
            da, da_off = (dx, 0) if blk == 0 else (gf, (blk - 1) * g0)
            grads = _dense_block_backward(a=a, a_off=a_off, ca=g0, layers=params[i0:i0 + per], need=need[i0:i0 + per],
                                          growth=growths[blk], gg=gg, dy=gf, dy_off=blk * g0, da=da, da_off=da_off,
                                          beta_a=0.0 if blk == 0 else 1.0, act=ACT_RELU, slope=0.0, terms=terms) + grads
        return (dx, None, None, None) + tuple(grads)


def residual_dense_blocks(x, blocks):
    """The trunk of RDN: D residual dense blocks without a concatenation.  x: [N, G0, H, W]; blocks: D sequences
    (w_1, b_1, ..., w_C, b_C, w_lff, b_lff) with w_c [G, G0 + (c - 1) G, 3, 3] and w_lff [G0, G0 + C G, 1, 1].  Returns the
    global-fusion buffer [N, D * G0, H, W] (channels_last) = cat(RDB_1 .. RDB_D outputs): block d writes channels
    [d G0, (d + 1) G0) and block d + 1 reads them in place.  C + 1 launches a block forward; the backward accumulates
    every gradient fan-in inside the data-gradient kernels (base_networks.RDB, models.RDNNet)."""
    blocks = [tuple(b) for b in blocks]
    if not blocks or len(set(len(b) for b in blocks)) != 1 or len(blocks[0]) < 4 or len(blocks[0]) % 2:
        raise ValueError("residual_dense_blocks: every block is (w_1, b_1, ..., w_C, b_C, w_lff, b_lff) with the same C >= 1")
    if x.dim() != 4:
        raise ValueError("residual_dense_blocks: x must be [N, G0, H, W], got shape %s" % (tuple(x.shape),))
    C = len(blocks[0]) // 2 - 1
    g0, g = int(x.shape[1]), int(blocks[0][0].shape[0])
    for b in blocks:
        for c in range(C):
            if tuple(b[2 * c].shape) != (g, g0 + c * g, 3, 3) or tuple(b[2 * c + 1].shape) != (g,):
                raise ValueError("residual_dense_blocks: layer %d holds %s / %s, expected [%d, %d, 3, 3] / [%d]"
                                 % (c + 1, tuple(b[2 * c].shape), tuple(b[2 * c + 1].shape), g, g0 + c * g, g))
        if tuple(b[2 * C].shape) != (g0, g0 + C * g, 1, 1) or tuple(b[2 * C + 1].shape) != (g0,):
            raise ValueError("residual_dense_blocks: the local fusion holds %s / %s, expected [%d, %d, 1, 1] / [%d]"
                             % (tuple(b[2 * C].shape), tuple(b[2 * C + 1].shape), g0, g0 + C * g, g0))
    for name, v in (("G0", g0), ("G", g)):
        if v % 16:
            raise ValueError("residual_dense_blocks: %s = %d is not a multiple of 16" % (name, v))
    if g > 64 or g0 > 64:
        raise ValueError("residual_dense_blocks: G = %d, G0 = %d: at most 64 output channels a convolution" % (g, g0))
    params = [t for b in blocks for t in b]
    return _ResidualDenseBlocks.apply(x, len(blocks), C, grad_enabled_for(x, *params), *params)


# ------------------------------------------------------------------------------------------------
# The residual-in-residual dense trunk of ESRGAN (csrc/dense.hip: the _ex entry points)
# The second buffer policy on the block core above: ping-pong trunk maps, scaled skips in the fusion epilogue.
# ------------------------------------------------------------------------------------------------
_RRDB_SLOPE = 0.2


def _trunk_buffer(n, c, h, w, like):
    """An RDB's output map (its own name, so that a test can count them)."""
    return _empty_cl(n, c, h, w, like)


class _RRDBTrunk(torch.autograd.Function):
    """nb residual-in-residual dense blocks on slice convolutions; see rrdb_trunk."""

    @staticmethod
    def forward(ctx, x, nb, rs, need_grad, *params):
        require_cuda(x, *params)
        x = to_nhwc(x)
        n, f, hh, ww = x.shape
        g = int(params[0].shape[0])
        terms = dense_terms("train_fwd" if need_grad else "infer")
        free, growth = [], None
        ins, growths = [], []

        def take():
            return free.pop() if free else _trunk_buffer(n, f, hh, ww, x)

        u1 = x
        for i in range(nb):
            u = u1
            for k in range(3):
                p = params[30 * i + 10 * k:30 * i + 10 * k + 10]
                if need_grad or growth is None:     # a backward reads every growth buffer: the LeakyReLU masks, the wgrad inputs
                    growth = _growth_buffer(n, 4 * g, hh, ww, x)
                v = _trunk_buffer(n, f, hh, ww, x) if need_grad else take()
                if k < 2:      # v = rs conv5 + u
                    skips = dict(s=rs, r1=1.0)
                else:          # out = rs (rs conv5 + u3) + u1: the outer skip rides in the same epilogue
                    skips = dict(s=rs * rs, r1=rs, residual2=u1, r2=1.0)
                _dense_block_forward(a=u, a_off=0, ca=f, layers=p, growth=growth, out=v, out_off=0, act=ACT_LRELU,
                                     slope=_RRDB_SLOPE, terms=terms, **skips)
                if need_grad:
                    ins.append(u)
                    growths.append(growth)
                elif k > 0:
                    free.append(u)                  # u2 / u3: read for the last time
                u = v
            if not need_grad and i > 0:
                free.append(u1)
            u1 = u
        ctx.dims = (nb, f, g, float(rs))
        ctx.params = params
        if need_grad:
            ctx.save_for_backward(*(ins + growths))
        return u1

    @staticmethod
    def backward(ctx, gout):
        nb, f, g, rs = ctx.dims
        params = ctx.params
        saved = ctx.saved_tensors
        ins, growths = saved[:3 * nb], saved[3 * nb:]
        n, _, hh, ww = ins[0].shape
        terms = dense_terms("bwd")
        like = ins[0]
        gnext = _dense(gout)               # read only: every accumulator below is this op's own
        gg = _empty_cl(n, 4 * g, hh, ww, like)
        need, grads = ctx.needs_input_grad[4:], [None] * len(params)

        def rdb(j, dy, da, s, a1, extra=None):
            """The backward of RDB j (its output = s conv5 + a1 u + ...): da = the whole gradient of its input u, written
            (beta 0); `extra`: the RRDB's outer skip."""
            grads[10 * j:10 * j + 10] = _dense_block_backward(
                a=ins[j], a_off=0, ca=f, layers=params[10 * j:10 * j + 10], need=need[10 * j:10 * j + 10], growth=growths[j],
                gg=gg, dy=dy, dy_off=0, da=da, da_off=0, beta_a=0.0, act=ACT_LRELU, slope=_RRDB_SLOPE, terms=terms, s=s,
                a1=a1, extra=extra)

        for i in reversed(range(nb)):
            gu3 = _empty_cl(n, f, hh, ww, like)
            rdb(3 * i + 2, gnext, gu3, s=rs * rs, a1=rs)            # out = rs^2 conv5 + rs u3 + u1
            gu2 = _empty_cl(n, f, hh, ww, like)
            rdb(3 * i + 1, gu3, gu2, s=rs, a1=1.0)                  # u3 = rs conv5 + u2
            gu1 = _empty_cl(n, f, hh, ww, like) if (i > 0 or ctx.needs_input_grad[0]) else None
            rdb(3 * i, gu2, gu1, s=rs, a1=1.0, extra=gnext)         # u2 = rs conv5 + u1, and u1's own way to the output
            gnext = gu1
        return (gnext, None, None, None) + tuple(grads)


def rrdb_trunk(x, blocks, res_scale=0.2):
    """The trunk of ESRGAN's RRDBNet: residual-in-residual dense blocks without a concatenation or an elementwise launch.
    x: [N, F, H, W]; blocks: a list of RRDBs, each 3 RDBs, each (w1, b1, ..., w5, b5) with w_c [G, F + (c - 1) G, 3, 3] for
    c = 1..4 and w5 [F, F + 4 G, 3, 3].  Per RDB: four slice convolutions with LeakyReLU(0.2) into one growth buffer, then
    u' = res_scale * conv5([u | growth]) + u; an RRDB's third conv5 also folds the outer skip into its epilogue:
    out = res_scale^2 * conv5 + res_scale * u3 + u1.  15 launches an RRDB forward; the backward (15 data-gradient and 15
    two-launch weight-gradient calls an RRDB) accumulates every fan-in inside the data-gradient epilogues.
    F and G: multiples of 16, at most 64 (ValueError otherwise).  (base_networks.RRDB, models.RRDBNet)"""
    blocks = [tuple(tuple(r) for r in b) for b in blocks]
    if x.dim() != 4:
        raise ValueError("rrdb_trunk: x must be [N, F, H, W], got shape %s" % (tuple(x.shape),))
    if not blocks or any(len(b) != 3 or any(len(r) != 10 for r in b) for b in blocks):
        raise ValueError("rrdb_trunk: every RRDB is 3 RDBs of (w1, b1, ..., w5, b5)")
    f, g = int(x.shape[1]), int(blocks[0][0][0].shape[0])
    for name, v in (("F", f), ("G", g)):
        if v % 16:
            raise ValueError("rrdb_trunk: %s = %d is not a multiple of 16" % (name, v))
        if v > 64:
            raise ValueError("rrdb_trunk: %s = %d: at most 64 output channels a convolution" % (name, v))
    if not 0.0 < float(res_scale) < float("inf"):
        raise ValueError("rrdb_trunk: res_scale = %r is not a positive number" % (res_scale,))
    for b in blocks:
        for r in b:
            for c in range(5):
                want = (g, f + c * g, 3, 3) if c < 4 else (f, f + 4 * g, 3, 3)
                if tuple(r[2 * c].shape) != want or tuple(r[2 * c + 1].shape) != want[:1]:
                    raise ValueError("rrdb_trunk: conv%d holds %s / %s, expected [%d, %d, 3, 3] / [%d]"
                                     % (c + 1, tuple(r[2 * c].shape), tuple(r[2 * c + 1].shape), want[0], want[1], want[0]))
    params = [t for b in blocks for r in b for t in r]
    return _RRDBTrunk.apply(x, len(blocks), float(res_scale), grad_enabled_for(x, *params), *params)


class _RaganLoss(torch.autograd.Function):
    """srk_ragan_loss_forward_backward: the loss and both gradient rows from one launch, under the losses' seed contract."""

    @staticmethod
    def forward(ctx, real, fake, for_generator):
        lib = _lib.load()
        require_cuda(real, fake)
        for name, t in (("real_logits", real), ("fake_logits", fake)):
            if not (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1)) or t.shape[0] < 1:
                raise ValueError("ragan_loss: %s must be [B] or [B, 1] with B >= 1, got shape %s" % (name, tuple(t.shape)))
        if real.shape[0] != fake.shape[0]:
            raise ValueError("ragan_loss: %d real logits vs %d fake" % (real.shape[0], fake.shape[0]))
        real, fake = real.contiguous(), fake.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=real.device)
        d_real = torch.empty_like(real) if ctx.needs_input_grad[0] else None
        d_fake = torch.empty_like(fake) if ctx.needs_input_grad[1] else None
        check(lib.srk_ragan_loss_forward_backward(ptr(real), ptr(fake), int(real.shape[0]), 1 if for_generator else 0,
                                                  _declare_seed(ctx), ptr(loss), ptr(d_real), ptr(d_fake), None, stream_ptr()),
              "srk_ragan_loss_forward_backward")
        ctx.grads = (d_real, d_fake)
        return loss

    @staticmethod
    def backward(ctx, g):
        return _seed_scaled(ctx, g, ctx.grads) + (None,)


def ragan_loss(real_logits, fake_logits, for_generator):
    """The relativistic average GAN loss of ESRGAN on discriminator LOGITS ([B] or [B, 1]): with a = real - mean(fake) and
    b = fake - mean(real), the discriminator's mean of softplus(-a) and softplus(b) or, for_generator, of softplus(a) and
    softplus(-b); the gradient is the full derivative, the means included.  A 0-dim fp32 device tensor under the seed
    contract of the losses (_declare_seed); a detached operand gets no gradient row.
    include/srk.h: srk_ragan_loss_forward_backward."""
    return _RaganLoss.apply(real_logits, fake_logits, bool(for_generator))


# ------------------------------------------------------------------------------------------------
# The operators of Real-ESRGAN's U-Net discriminator: spectral normalisation, bilinear x2, the vanilla GAN loss on logits
# (csrc/spectral_norm.hip, csrc/bilinear.hip, csrc/gan_logit.hip)
# ------------------------------------------------------------------------------------------------
SPECTRAL_EPS = 1e-12


class _SpectralForward(object):
    """What one layer's backward reads of the forward it belongs to: its own w_sn and its own copy of (u, v, sigma)."""
    __slots__ = ("w_sn", "saved", "R", "K")


def _spectral_forward_raw(layers, training):
    """One srk_spectral_norm_forward call for all `layers` = [(weight_orig, u, v), ...] -> [_SpectralForward, ...]."""
    lib = _lib.load()
    if not 1 <= len(layers) <= _lib.SPECTRAL_MAX_LAYERS:
        raise ValueError("spectral_norm: %d layers, 1 .. %d go into one call" % (len(layers), _lib.SPECTRAL_MAX_LAYERS))
    table = (_lib.SpectralLayer * len(layers))()
    outs = []
    for i, (w, u, v) in enumerate(layers):
        require_cuda(w, u, v)
        if w.dim() < 2 or not w.is_contiguous():
            raise ValueError("spectral_norm: layer %d: the weight must be dense with at least two axes, got shape %s"
                             % (i, tuple(w.shape)))
        R, K = int(w.shape[0]), int(w.numel() // w.shape[0])
        if tuple(u.shape) != (R,) or tuple(v.shape) != (K,) or not u.is_contiguous() or not v.is_contiguous():
            raise ValueError("spectral_norm: layer %d: u %s / v %s do not match the [%d, %d] view of the weight"
                             % (i, tuple(u.shape), tuple(v.shape), R, K))
        f = _SpectralForward()
        f.R, f.K = R, K
        f.w_sn = torch.empty(w.shape, dtype=torch.float32, device=w.device)
        f.saved = torch.empty(R + K + 1, dtype=torch.float32, device=w.device)
        table[i] = _lib.SpectralLayer(w.data_ptr(), u.data_ptr(), v.data_ptr(), f.w_sn.data_ptr(), f.saved.data_ptr(), R, K)
        outs.append(f)
    nbytes = int(lib.srk_spectral_norm_workspace(table, len(layers)))
    if nbytes == 0:
        raise RuntimeError("spectral_norm: %s" % lib.srk_last_error_string().decode())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=layers[0][0].device)
    check(lib.srk_spectral_norm_forward(table, len(layers), 1 if training else 0, SPECTRAL_EPS, ptr(ws), ws.numel(),
                                        stream_ptr()), "srk_spectral_norm_forward")
    return outs


class _SpectralNormNode(torch.autograd.Function):
    """The autograd node of ONE layer of a multi-layer spectral_norm call: forward hands out the w_sn the call computed,
    backward turns G = dL/dw_sn into dW with the u, v, sigma of that forward (srk_spectral_norm_backward, two launches).
    With a flat gradient buffer (optim.FlatParams) dW is accumulated into the parameter's slice, beta = 1."""

    @staticmethod
    def forward(ctx, weight_orig, fwd):
        ctx.fwd, ctx.weight_ref = fwd, weight_orig
        return fwd.w_sn

    @staticmethod
    def backward(ctx, G):
        lib = _lib.load()
        f, w = ctx.fwd, ctx.weight_ref
        G = G.contiguous()
        acc = getattr(w, "_srk_grad", None)
        dW, beta = (acc, 1.0) if acc is not None else (torch.empty_like(f.w_sn), 0.0)
        ws = torch.empty(max(int(lib.srk_spectral_norm_backward_workspace(f.R, f.K)), 8), dtype=torch.uint8, device=G.device)
        check(lib.srk_spectral_norm_backward(ptr(G), ptr(f.w_sn), ptr(f.saved), f.R, f.K, ptr(dW), beta, ptr(ws), ws.numel(),
                                             stream_ptr()), "srk_spectral_norm_backward")
        return (None if acc is not None else dW), None


def spectral_norm(layers, training=True):
    """torch.nn.utils.spectral_norm(n_power_iterations=1, eps=1e-12, dim=0) for a list of layers [(weight_orig, u, v), ...]
    in ONE call of three launches (two in eval mode): training mode runs one power iteration and writes u and v back in
    place; then sigma = u . (W v) and w_sn = W / sigma.  Returns the list of w_sn, ordinary non-leaf tensors to hand to
    ops.conv2d: each has its own backward node (u, v constants, as in torch), which keeps the u, v, sigma of this call.  A
    weight_orig that does not require a gradient (a frozen discriminator) gets a plain tensor and no node.
    include/srk.h: srk_spectral_norm_forward / _backward."""
    outs = _spectral_forward_raw([(w.detach(), u, v) for w, u, v in layers], training)
    res = []
    for (w, _, _), f in zip(layers, outs):
        if torch.is_grad_enabled() and w.requires_grad:
            res.append(_SpectralNormNode.apply(w, f))
        else:
            res.append(f.w_sn)
    return res


class _UpsampleBilinear2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, add):
        lib = _lib.load()
        require_cuda(x, add)
        if x.dim() != 4:
            raise ValueError("upsample_bilinear2x: takes [N, C, H, W], got shape %s" % (tuple(x.shape),))
        if add is not None and add.shape != x.shape:
            raise ValueError("upsample_bilinear2x: add %s does not match x %s" % (tuple(add.shape), tuple(x.shape)))
        x = to_nhwc(x)
        add = to_nhwc(add) if add is not None else None
        n, c, h, w = x.shape
        y = _empty_cl(n, c, 2 * h, 2 * w, x)
        check(lib.srk_upsample_bilinear2x_forward(ptr(x), ptr(add), ptr(y), n, h, w, c, stream_ptr()),
              "srk_upsample_bilinear2x_forward")
        ctx.has_add = add is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        dy = _dense(dy)
        n, c, hr, wr = dy.shape
        dx = _empty_cl(n, c, hr // 2, wr // 2, dy)
        check(lib.srk_upsample_bilinear2x_backward(ptr(dy), ptr(dx), n, hr // 2, wr // 2, c, stream_ptr()),
              "srk_upsample_bilinear2x_backward")
        return (dx if ctx.needs_input_grad[0] else None), (dx if ctx.has_add and ctx.needs_input_grad[1] else None)


def upsample_bilinear2x(x, add=None):
    """F.interpolate(x + add, scale_factor=2, mode='bilinear', align_corners=False) in one launch; `add` (a U-Net skip) is
    summed while x is read.  The backward is the adjoint in gather form, one launch; its result is the gradient of x and
    of add alike (the same tensor).  include/srk.h: srk_upsample_bilinear2x_forward / _backward."""
    return _UpsampleBilinear2x.apply(x, add)


class _GanLogitLoss(torch.autograd.Function):
    """srk_gan_logit_loss_forward_backward: loss and gradient from one pass and a finish, under the losses' seed contract."""

    @staticmethod
    def forward(ctx, logits, target_is_real):
        lib = _lib.load()
        require_cuda(logits)
        if logits.numel() < 1:
            raise ValueError("gan_logit_loss: no logits (shape %s)" % (tuple(logits.shape),))
        x = logits if (logits.is_contiguous() or (logits.dim() == 4 and _is_nhwc_dense(logits))) else logits.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None     # (preserve_format: the storage order of x)
        ws = torch.empty(int(lib.srk_gan_logit_loss_workspace_bytes()), dtype=torch.uint8, device=x.device)
        check(lib.srk_gan_logit_loss_forward_backward(ptr(x), x.numel(), 1 if target_is_real else 0, _declare_seed(ctx),
                                                      ptr(loss), ptr(dx), ptr(ws), stream_ptr()),
              "srk_gan_logit_loss_forward_backward")
        ctx.grads = (dx,)
        return loss

    @staticmethod
    def backward(ctx, g):
        return _seed_scaled(ctx, g, ctx.grads) + (None,)


def gan_logit_loss(logits, target_is_real):
    """The vanilla GAN loss on discriminator LOGITS of any shape (a U-Net discriminator's [B, 1, H, W] map, or [B, 1]):
    mean softplus(-x) for a real target, mean softplus(x) for a fake one (BCEWithLogits against ones / zeros).  A 0-dim
    fp32 device tensor under the seed contract of the losses (_declare_seed).
    include/srk.h: srk_gan_logit_loss_forward_backward."""
    return _GanLogitLoss.apply(logits, bool(target_is_real))


# ------------------------------------------------------------------------------------------------
# Motion compensation: flow warp, early fusion, flow smoothness (csrc/mc.hip, csrc/mc_common.h)
# ------------------------------------------------------------------------------------------------
def _flow_arg(who, flow, rows, h, w):
    """A flow [rows,2,H,W] as the kernels read it: either dense memory format as it is, anything else copied."""
    if flow.dim() != 4 or tuple(flow.shape) != (rows, 2, h, w) or flow.dtype != torch.float32:
        raise ValueError("%s: flow must be fp32 [%d,2,%d,%d] (x then y displacement, in pixels), got %s %s"
                         % (who, rows, h, w, flow.dtype, tuple(flow.shape)))
    return flow if (_is_nchw_dense(flow) or _is_nhwc_dense(flow)) else flow.contiguous()


def _no_image_grad(who, name, img):
    if img.requires_grad:
        raise ValueError("%s: `%s` requires a gradient, but the warped image is a data frame: the gradient goes to the flow "
                         "only (its adjoint would be a scatter); pass %s.detach()" % (who, name, name))


class _FlowWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, flow):
        n, c, h, w = img.shape
        out = _empty_cl(n, c, h, w, img)
        check(_lib.load().srk_flow_warp_forward(ptr(img), _strides4(img), ptr(flow), _strides4(flow), n, c, h, w, ptr(out),
                                                stream_ptr()), "srk_flow_warp_forward")
        ctx.save_for_backward(img, flow)
        return out

    @staticmethod
    def backward(ctx, g):
        img, flow = ctx.saved_tensors
        n, c, h, w = img.shape
        dflow = torch.empty_like(flow)
        check(_lib.load().srk_flow_warp_backward(ptr(img), _strides4(img), ptr(flow), _strides4(flow), ptr(g), _strides4(g),
                                                 n, c, h, w, ptr(dflow), _strides4(dflow), stream_ptr()),
              "srk_flow_warp_backward")
        return None, dflow


def flow_warp(img, flow):
    """img [N,C,H,W] sampled bilinearly at (x + flow[:,0], y + flow[:,1]), in pixels, coordinates clamped to the picture:
    F.grid_sample(mode='bilinear', padding_mode='border', align_corners=True) on pixel coordinates, one launch, the result
    channels_last.  The gradient goes to the flow only (one launch; on an integer coordinate the right-hand cell's slope,
    0 where the unclamped coordinate leaves the picture); an img that requires one is a ValueError.
    include/srk_mc.h: srk_flow_warp_forward / _backward."""
    if img.dim() != 4 or img.dtype != torch.float32 or img.numel() == 0:
        raise ValueError("flow_warp: img must be a non-empty fp32 [N,C,H,W] tensor, got %s %s" % (img.dtype, tuple(img.shape)))
    _no_image_grad("flow_warp", "img", img)
    require_cuda(img, flow)
    n, c, h, w = img.shape
    flow = _flow_arg("flow_warp", flow, n, h, w)
    return _FlowWarp.apply(img, flow)    # (img is read through its strides: a channel slice of a batch is not copied)


class _MotionFuse(torch.autograd.Function):
    """srk_motion_fuse_forward / _backward.  The mc loss follows the seed contract of the losses: its own seed (the unit
    seed, or the one declared by loss_seed) is a host factor of the backward launch, any other upstream gradient a
    device scalar the same launch reads -- no scale pass either way."""

    @staticmethod
    def forward(ctx, frames, flow):
        lib = _lib.load()
        n, _, c, h, w = frames.shape
        fused = _empty_cl(n, 3 * c, h, w, frames)
        loss = torch.empty((), dtype=torch.float32, device=frames.device)
        ws = torch.empty(int(lib.srk_mc_workspace_bytes()), dtype=torch.uint8, device=frames.device)
        check(lib.srk_motion_fuse_forward(ptr(frames), ptr(flow), _strides4(flow), n, c, h, w, ptr(fused), ptr(loss), ptr(ws),
                                          stream_ptr()), "srk_motion_fuse_forward")
        _declare_seed(ctx)
        ctx.set_materialize_grads(False)   # an unused output's gradient arrives as None, not as a zeros fill
        ctx.save_for_backward(frames, flow)
        return fused, loss

    @staticmethod
    def backward(ctx, g_fused, g_mc):
        frames, flow = ctx.saved_tensors
        n, _, c, h, w = frames.shape
        if g_mc is None:
            seed, seed_dev = 0.0, None
        elif _is_own_seed(ctx, g_mc, frames.device):
            seed, seed_dev = ctx.seed_value, None
        else:
            seed, seed_dev = 1.0, g_mc.reshape(()).to(torch.float32)
        dflow = torch.empty_like(flow)
        check(_lib.load().srk_motion_fuse_backward(ptr(frames), ptr(flow), _strides4(flow), ptr(g_fused),
                                                   None if g_fused is None else _strides4(g_fused), n, c, h, w, seed,
                                                   ptr(seed_dev), ptr(dflow), _strides4(dflow), stream_ptr()),
              "srk_motion_fuse_backward")
        return None, dflow


def motion_fuse(frames, flow):
    """VESPCN's early fusion with its motion-compensation loss, one pass: frames [N,3,C,H,W] (t-1, t, t+1), flow
    [2N,2,H,W] in pixels (rows 0..N-1 move frame t-1 onto t, rows N..2N-1 frame t+1) ->
      fused [N,3C,H,W] channels_last = [flow_warp(t-1) | frame t | flow_warp(t+1)],
      mc = mean over all 2 N C H W elements of (warped - frame t)^2, a 0-dim fp32 tensor under the losses' seed contract.
    The gradient goes to the flow only, in one launch that recomputes the samples; frames that require one are a
    ValueError.  include/srk_mc.h: srk_motion_fuse_forward / _backward."""
    if frames.dim() != 5 or frames.shape[1] != 3 or frames.dtype != torch.float32 or frames.numel() == 0:
        raise ValueError("motion_fuse: frames must be a non-empty fp32 [N,3,C,H,W] tensor (t-1, t, t+1), got %s %s"
                         % (frames.dtype, tuple(frames.shape)))
    _no_image_grad("motion_fuse", "frames", frames)
    require_cuda(frames, flow)
    n, _, c, h, w = frames.shape
    flow = _flow_arg("motion_fuse", flow, 2 * n, h, w)
    return _MotionFuse.apply(frames.contiguous(), flow)


class _FlowHuber(torch.autograd.Function):
    """srk_flow_huber_forward_backward: loss and gradient from one pass and a finish, under the losses' seed contract."""

    @staticmethod
    def forward(ctx, flow, eps):
        lib = _lib.load()
        m, _, h, w = flow.shape
        loss = torch.empty((), dtype=torch.float32, device=flow.device)
        dflow = torch.empty_like(flow) if ctx.needs_input_grad[0] else None   # (preserve_format: stored like the flow)
        ws = torch.empty(int(lib.srk_mc_workspace_bytes()), dtype=torch.uint8, device=flow.device)
        check(lib.srk_flow_huber_forward_backward(ptr(flow), _strides4(flow), m, h, w, eps, _declare_seed(ctx), ptr(loss),
                                                  ptr(dflow), ptr(ws), stream_ptr()), "srk_flow_huber_forward_backward")
        ctx.grads = (dflow,)
        return loss

    @staticmethod
    def backward(ctx, g):
        return _seed_scaled(ctx, g, ctx.grads) + (None,)


def flow_huber_loss(flow, eps=0.01):
    """The flow-smoothness term of VESPCN, per pixel: mean over M H W of sqrt(eps + dx_u^2 + dy_u^2 + dx_v^2 + dy_v^2) with
    the forward differences of both components of flow [M,2,H,W] (0 at the last column and row).  A 0-dim fp32 device
    tensor under the seed contract of the losses (_declare_seed).  include/srk_mc.h: srk_flow_huber_forward_backward."""
    require_cuda(flow)
    if flow.dim() != 4 or flow.numel() == 0:
        raise ValueError("flow_huber_loss: flow must be a non-empty [M,2,H,W] tensor, got %s" % (tuple(flow.shape),))
    if not float(eps) > 0.0:
        raise ValueError("flow_huber_loss: eps %r is not positive" % (eps,))
    m, _, h, w = flow.shape
    return _FlowHuber.apply(_flow_arg("flow_huber_loss", flow, m, h, w), float(eps))


def _host_flow(who, flow, rows, h, w):
    flow = np.asarray(flow)
    if flow.dtype != np.float32 or flow.shape != (rows, 2, h, w) or any(s % 4 or s < 0 for s in flow.strides):
        raise ValueError("%s: flow must be a float32 [%d,2,%d,%d] array, got %s %s" % (who, rows, h, w, flow.dtype, flow.shape))
    return flow, (ctypes.c_int64 * 4)(*[s // 4 for s in flow.strides])


def _host_grad(who, g, shape):
    if g is None:
        return None
    g = np.ascontiguousarray(g, dtype=np.float64)
    if g.shape != shape:
        raise ValueError("%s: the upstream gradient must be %s, got %s" % (who, shape, g.shape))
    return g


def flow_warp_host(img, flow, g=None):
    """flow_warp on host memory in double (srk_flow_warp_host: the kernels' per-pixel header in plain C++): numpy float32
    img [N,C,H,W] and flow [N,2,H,W] of any strides -> (out, dflow), float64 NCHW; dflow is for the upstream gradient g
    ([N,C,H,W]; None: zeros)."""
    img = np.asarray(img)
    if img.dtype != np.float32 or img.ndim != 4 or img.size == 0 or any(s % 4 or s < 0 for s in img.strides):
        raise ValueError("flow_warp_host: img must be a non-empty float32 [N,C,H,W] array, got %s %s" % (img.dtype, img.shape))
    n, c, h, w = img.shape
    flow, fs = _host_flow("flow_warp_host", flow, n, h, w)
    g = _host_grad("flow_warp_host", g, (n, c, h, w))
    out, dflow = np.empty((n, c, h, w), dtype=np.float64), np.empty((n, 2, h, w), dtype=np.float64)
    check(_lib.load().srk_flow_warp_host(_np_ptr(img), (ctypes.c_int64 * 4)(*[s // 4 for s in img.strides]), _np_ptr(flow), fs,
                                         n, c, h, w, _np_ptr(g), _np_ptr(out), _np_ptr(dflow)), "srk_flow_warp_host")
    return out, dflow


def motion_fuse_host(frames, flow, g_fused=None, seed=1.0):
    """motion_fuse on host memory in double (srk_motion_fuse_host): numpy float32 frames [N,3,C,H,W] and flow [2N,2,H,W]
    -> (fused [N,3C,H,W], mc, dflow [2N,2,H,W]), float64; dflow is the gradient of sum(g_fused * fused) + seed * mc."""
    frames = np.ascontiguousarray(frames)
    if frames.dtype != np.float32 or frames.ndim != 5 or frames.shape[1] != 3 or frames.size == 0:
        raise ValueError("motion_fuse_host: frames must be a non-empty float32 [N,3,C,H,W] array, got %s %s"
                         % (frames.dtype, frames.shape))
    n, _, c, h, w = frames.shape
    flow, fs = _host_flow("motion_fuse_host", flow, 2 * n, h, w)
    g = _host_grad("motion_fuse_host", g_fused, (n, 3 * c, h, w))
    fused, dflow = np.empty((n, 3 * c, h, w), dtype=np.float64), np.empty((2 * n, 2, h, w), dtype=np.float64)
    loss = ctypes.c_double()
    check(_lib.load().srk_motion_fuse_host(_np_ptr(frames), _np_ptr(flow), fs, n, c, h, w, float(seed), _np_ptr(g),
                                           _np_ptr(fused), ctypes.byref(loss), _np_ptr(dflow)), "srk_motion_fuse_host")
    return fused, loss.value, dflow


def flow_huber_host(flow, eps=0.01, grad_scale=1.0):
    """flow_huber_loss on host memory in double (srk_flow_huber_host) -> (loss, grad_scale * d loss / d flow)."""
    flow = np.asarray(flow)
    if flow.ndim != 4 or flow.size == 0:
        raise ValueError("flow_huber_host: flow must be a non-empty [M,2,H,W] array, got %s" % (flow.shape,))
    m, _, h, w = flow.shape
    flow, fs = _host_flow("flow_huber_host", flow, m, h, w)
    dflow = np.empty((m, 2, h, w), dtype=np.float64)
    loss = ctypes.c_double()
    check(_lib.load().srk_flow_huber_host(_np_ptr(flow), fs, m, h, w, float(eps), float(grad_scale), ctypes.byref(loss),
                                          _np_ptr(dflow)), "srk_flow_huber_host")
    return loss.value, dflow


# ------------------------------------------------------------------------------------------------
# SwinIR's operators: shifted-window attention, LayerNorm, GELU (csrc/wattn.hip, csrc/swin_pointwise.hip)
# ------------------------------------------------------------------------------------------------
WATTN_MAX_HEAD_DIM = _lib.WATTN_MAX_HEAD_DIM


def window_attention_check(c, heads, window, shift, h=None, w=None, who="window_attention"):
    """The shapes the kernel covers; anything else is a ValueError that names the number."""
    if not 2 <= int(window) <= 8:
        raise ValueError("%s: window %r is not in 2 .. 8 (one lane per token, window^2 <= 64)" % (who, window))
    if not 0 <= int(shift) < int(window):
        raise ValueError("%s: shift %r is not in 0 .. window - 1 = %d" % (who, shift, window - 1))
    if heads < 1 or c % heads:
        raise ValueError("%s: %r heads do not divide %d channels" % (who, heads, c))
    if c // heads > WATTN_MAX_HEAD_DIM:
        raise ValueError("%s: head dimension %d = %d / %d exceeds %d" % (who, c // heads, c, heads, WATTN_MAX_HEAD_DIM))
    if h is not None and (h % window or w % window):
        raise ValueError("%s: a %d x %d map is not a multiple of the window %d" % (who, h, w, window))


class _WindowAttention(torch.autograd.Function):
    """softmax(d^-0.5 Q K^T + bias + mask) V per shifted window and head on an NHWC map: one launch forward, two
    backward; saves qkv, the output and the row log-sum-exp."""

    @staticmethod
    def forward(ctx, qkv, table, heads, window, shift):
        lib = _lib.load()
        require_cuda(qkv, table)
        n, h, w, c3 = qkv.shape
        c = c3 // 3
        qkv = qkv.contiguous()
        tb = table.detach().contiguous()
        need_grad = any(ctx.needs_input_grad)
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=qkv.device)
        lse = None
        if need_grad:
            lse = torch.empty((n * (h // window) * (w // window), heads, 64), dtype=torch.float32, device=qkv.device)
        check(lib.srk_window_attention_forward(ptr(qkv), ptr(tb), n, h, w, c, heads, window, shift, ptr(out), ptr(lse),
                                               stream_ptr()), "srk_window_attention_forward")
        ctx.cfg = (heads, window, shift)
        ctx.table_ref = table
        if need_grad:
            ctx.save_for_backward(qkv, tb, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        qkv, tb, out, lse = ctx.saved_tensors
        heads, window, shift = ctx.cfg
        n, h, w, c3 = qkv.shape
        c = c3 // 3
        dout = dout.contiguous()      # a strided gradient is copied, never read with the wrong strides
        dqkv = torch.empty_like(qkv)
        dtable = ret = ws = None
        beta, nbytes = 0.0, 0
        if ctx.needs_input_grad[1]:
            dtable = getattr(ctx.table_ref, "_srk_grad", None)   # optim.FlatParams: accumulate into the flat buffer
            if dtable is not None:
                beta = 1.0
            else:
                dtable = ret = torch.empty(tb.shape, dtype=torch.float32, device=qkv.device)
            nbytes = int(lib.srk_window_attention_workspace(n, h, w, c, heads, window))
            ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=qkv.device)
        check(lib.srk_window_attention_backward(ptr(dout), ptr(qkv), ptr(tb), ptr(out), ptr(lse), n, h, w, c, heads, window,
                                                shift, ptr(dqkv), ptr(dtable), beta, ptr(ws), nbytes, stream_ptr()),
              "srk_window_attention_backward")
        return dqkv if ctx.needs_input_grad[0] else None, ret, None, None, None


def window_attention(qkv, table, heads, window, shift=0):
    """Shifted-window self-attention (Swin / SwinIR) on an NHWC map.  qkv [N, H, W, 3C]: the qkv projection with its bias,
    channels q | k | v, each heads x d; table [(2 window - 1)^2, heads]: the relative position bias.  Returns
    [N, H, W, C].  The roll by -shift, the window partition, the bias gather, the -100 mask of the shifted windows, the
    softmax and all their inverses are one kernel; nothing but the result is written.  include/srk.h:
    srk_window_attention_forward / _backward."""
    if qkv.dim() != 4 or qkv.shape[3] % 3:
        raise ValueError("window_attention: qkv must be [N, H, W, 3C], got shape %s" % (tuple(qkv.shape),))
    heads, window, shift = int(heads), int(window), int(shift)
    n, h, w, c3 = qkv.shape
    window_attention_check(c3 // 3, heads, window, shift, h, w)
    if tuple(table.shape) != ((2 * window - 1) ** 2, heads):
        raise ValueError("window_attention: table %s, expected (%d, %d) for window %d and %d heads"
                         % (tuple(table.shape), (2 * window - 1) ** 2, heads, window, heads))
    return _WindowAttention.apply(qkv, table, heads, window, shift)


def _ln_workspace(lib, rows, c, device):
    nbytes = int(lib.srk_layer_norm_workspace(rows, c))
    return torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device), nbytes


class _LayerNorm(torch.autograd.Function):
    """LayerNorm over the last axis with gamma and beta; saves x, mean and rstd per row."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        lib = _lib.load()
        require_cuda(x, gamma, beta)
        x = x.contiguous()
        c = x.shape[-1]
        rows = x.numel() // c
        gc, bc = gamma.detach().contiguous(), beta.detach().contiguous()
        need_grad = any(ctx.needs_input_grad)
        y = torch.empty_like(x)
        mean = rstd = None
        if need_grad:
            mean = torch.empty(rows, dtype=torch.float32, device=x.device)
            rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        check(lib.srk_layer_norm_forward(ptr(x), ptr(gc), ptr(bc), ptr(y), ptr(mean), ptr(rstd), rows, c, eps, stream_ptr()),
              "srk_layer_norm_forward")
        ctx.params = (gamma, beta)
        if need_grad:
            ctx.save_for_backward(x, gc, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, gc, mean, rstd = ctx.saved_tensors
        gamma, beta = ctx.params
        c = x.shape[-1]
        rows = x.numel() // c
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        need = ctx.needs_input_grad[1:3]
        acc = [getattr(p, "_srk_grad", None) for p in (gamma, beta)]
        flat = all(a is not None for a in acc)     # optim.FlatParams: accumulate into the flat gradient buffer
        if flat:
            outs, a = [g if nd else None for g, nd in zip(acc, need)], 1.0
        else:
            outs, a = [torch.empty(c, dtype=torch.float32, device=x.device) if nd else None for nd in need], 0.0
        ws, nbytes = _ln_workspace(lib, rows, c, x.device) if any(need) else (None, 0)
        check(lib.srk_layer_norm_backward(ptr(dy), ptr(x), ptr(gc), ptr(mean), ptr(rstd), ptr(dx), ptr(outs[0]),
                                          ptr(outs[1]), a, rows, c, ptr(ws), nbytes, stream_ptr()),
              "srk_layer_norm_backward")
        if flat:
            outs = [None, None]
        return dx, outs[0], outs[1], None


def layer_norm(x, gamma, beta, eps=1e-5):
    """nn.LayerNorm(C) over the last axis of a dense [..., C] tensor (an NHWC map or [rows, C]), any C >= 1."""
    if x.dim() < 1 or gamma.numel() != x.shape[-1] or beta.numel() != x.shape[-1]:
        raise ValueError("layer_norm: gamma %s and beta %s do not fit the last axis of %s"
                         % (tuple(gamma.shape), tuple(beta.shape), tuple(x.shape)))
    return _LayerNorm.apply(x, gamma, beta, float(eps))


def layer_norm_stats(x, gamma, beta, eps=1e-5):
    """(y, mean, rstd) of the forward kernel, without a graph: what the backward is given."""
    lib = _lib.load()
    require_cuda(x, gamma, beta)
    x = x.contiguous()
    c = x.shape[-1]
    rows = x.numel() // c
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(lib.srk_layer_norm_forward(ptr(x), ptr(gamma.detach().contiguous()), ptr(beta.detach().contiguous()), ptr(y),
                                     ptr(mean), ptr(rstd), rows, c, float(eps), stream_ptr()), "srk_layer_norm_forward")
    return y, mean, rstd


class _Gelu(torch.autograd.Function):
    """x Phi(x), the exact erf form; the backward reads the saved input."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        require_cuda(x)
        x = x.contiguous()      # (a view at an odd offset stays a view: the kernels have a 4-byte form)
        y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        check(lib.srk_gelu_forward(ptr(x), ptr(y), x.numel(), stream_ptr()), "srk_gelu_forward")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        check(lib.srk_gelu_backward(ptr(dy), ptr(x), ptr(dx), x.numel(), stream_ptr()), "srk_gelu_backward")
        return dx


def gelu(x):
    """nn.GELU() (approximate='none') on a dense tensor of any shape."""
    if x.numel() == 0:
        raise ValueError("gelu: empty tensor")
    return _Gelu.apply(x)


# -------------------------------------------------------------------------------------------------------------------------
# NIQE (Mittal, Soundararajan, Bovik 2013, as BasicSR's calculate_niqe states it; csrc/niqe.hip)
# -------------------------------------------------------------------------------------------------------------------------
_NIQE_TABLES = {}


def niqe_tables_host():
    """The three host-made tables of the AGGD fit as a float64 numpy array [3, 9801] over gam = 0.2 + 0.001 j: r_gam,
    sqrt(Gamma(1/g) / Gamma(3/g)), Gamma(2/g) / Gamma(1/g).  include/srk.h: srk_niqe_tables_host."""
    if "host" not in _NIQE_TABLES:
        out = np.empty((3, _lib.NIQE_TABLE), dtype=np.float64)
        check(_lib.load().srk_niqe_tables_host(out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "srk_niqe_tables_host")
        _NIQE_TABLES["host"] = out
    return _NIQE_TABLES["host"]


def niqe_tables(device=None):
    """niqe_tables_host() on the device, uploaded once per device."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev not in _NIQE_TABLES:
        _NIQE_TABLES[dev] = torch.from_numpy(niqe_tables_host()).to(dev)
    return _NIQE_TABLES[dev]


def _niqe_picture(img, who):
    """[C,H,W] (or [1,C,H,W]) float32 or uint8 of any strides -> (tensor [C,H,W], is_u8, (c, h, w) strides, C, H, W)."""
    if img.dim() == 4 and img.shape[0] == 1:
        img = img[0]
    if img.dim() != 3 or img.shape[0] not in (1, 3):
        raise ValueError("%s: takes one picture [C, H, W] with C in {1, 3}, got shape %s" % (who, tuple(img.shape)))
    if img.dtype not in (torch.float32, torch.uint8):
        raise ValueError("%s: takes a float32 or a uint8 picture, got %s" % (who, img.dtype))
    img = img.detach()
    strides = (ctypes.c_int64 * 3)(*[int(v) for v in img.stride()])
    return img, int(img.dtype == torch.uint8), strides, int(img.shape[0]), int(img.shape[1]), int(img.shape[2])


def niqe_blocks(h, w, shave=0, block=96):
    """(nh, nw): the grid of block x block blocks NIQE reads of an h x w picture with `shave` pixels off each side."""
    return max(int(h) - 2 * int(shave), 0) // int(block), max(int(w) - 2 * int(shave), 0) // int(block)


def _niqe_check(h, w, shave, block, who):
    shave, block = int(shave), int(block)
    if shave < 0:
        raise ValueError("%s: negative shave (%d)" % (who, shave))
    if block % 2 or not 8 <= block <= 96:
        raise ValueError("%s: block must be even and in 8 .. 96 (got %d)" % (who, block))
    nh, nw = niqe_blocks(h, w, shave, block)
    if nh * nw < 2:
        raise ValueError("%s: a picture of %d x %d with %d pixels shaved from each side holds %d x %d blocks of %d x %d, "
                         "fewer than 2" % (who, h, w, shave, nh, nw, block, block))
    return shave, block, nh * nw


def niqe_features(img, shave=0, block=96, sharpness=False):
    """NIQE's natural-scene-statistics features of one picture on the device: a float64 device tensor [blocks, 36] (18
    per scale; a block without both signs in a map holds NaNs there), and with sharpness=True also [blocks], the mean
    local sigma of each block at scale 1.  img: [C, H, W], C in {1, 3}, on the device, read in place through its strides
    -- float32 (quantised like to_u8_image on the way) or uint8.  Luma, crop, both scales and the AGGD fit run in two
    launches; nothing syncs.  include/srk.h: srk_niqe_features."""
    lib = _lib.load()
    img, is_u8, strides, c, h, w = _niqe_picture(img, "niqe_features")
    if not img.is_cuda:
        raise RuntimeError("niqe_features: the picture must be on the device (got %s); niqe_features_host is the "
                           "definition on host memory" % img.device)
    if img.device.index != torch.cuda.current_device():
        raise RuntimeError("niqe_features: tensor on %s but the current device is cuda:%d"
                           % (img.device, torch.cuda.current_device()))
    shave, block, blocks = _niqe_check(h, w, shave, block, "niqe_features")
    tables = niqe_tables(img.device)
    feats = torch.empty((blocks, _lib.NIQE_FEATURES), dtype=torch.float64, device=img.device)
    sharp = torch.empty(blocks, dtype=torch.float64, device=img.device) if sharpness else None
    ws = torch.empty(int(lib.srk_niqe_workspace_bytes(h, w, block)) // 8, dtype=torch.float64, device=img.device)
    check(lib.srk_niqe_features(ptr(img), is_u8, strides, c, h, w, shave, block, ptr(tables), ptr(feats), ptr(sharp),
                                ptr(ws), stream_ptr()), "srk_niqe_features")
    return (feats, sharp) if sharpness else feats


def niqe_features_host(img, shave=0, block=96, sharpness=False):
    """niqe_features in plain C++ double on host memory (srk_niqe_features_host): img is a CPU tensor or a numpy array
    [C, H, W], float32 or uint8, of any strides; returns numpy float64 arrays.  No device involved."""
    lib = _lib.load()
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(img)
    img, is_u8, strides, c, h, w = _niqe_picture(img, "niqe_features_host")
    if img.is_cuda:
        raise RuntimeError("niqe_features_host: takes host memory, got a tensor on %s" % img.device)
    shave, block, blocks = _niqe_check(h, w, shave, block, "niqe_features_host")
    tables = niqe_tables_host()
    feats = np.empty((blocks, _lib.NIQE_FEATURES), dtype=np.float64)
    sharp = np.empty(blocks, dtype=np.float64) if sharpness else None
    check(lib.srk_niqe_features_host(ctypes.c_void_p(img.data_ptr()), is_u8, strides, c, h, w, shave, block,
                                     tables.ctypes.data_as(ctypes.c_void_p), feats.ctypes.data_as(ctypes.c_void_p),
                                     sharp.ctypes.data_as(ctypes.c_void_p) if sharpness else None),
          "srk_niqe_features_host")
    return (feats, sharp) if sharpness else feats


def niqe_finish(features, mu_p, cov_p):
    """NIQE's score from the features of one picture and the pristine model (host, numpy, double): with mu = nanmean of
    the rows and cov = np.cov of the rows without a NaN, sqrt((mu_p - mu) pinv((cov_p + cov) / 2) (mu_p - mu)^T).
    features: [blocks, 36], a tensor (copied to the host here: the one sync) or an array."""
    f = features.detach().cpu().numpy() if torch.is_tensor(features) else np.asarray(features)
    f = np.asarray(f, dtype=np.float64)
    mu_p = np.asarray(mu_p, dtype=np.float64).reshape(-1)
    cov_p = np.asarray(cov_p, dtype=np.float64)
    nf = _lib.NIQE_FEATURES
    if f.ndim != 2 or f.shape[1] != nf or mu_p.shape != (nf,) or cov_p.shape != (nf, nf):
        raise ValueError("niqe_finish: features %s, mu_p %s, cov_p %s are not [blocks, %d], [%d], [%d, %d]"
                         % (f.shape, mu_p.shape, cov_p.shape, nf, nf, nf, nf))
    good = f[~np.isnan(f).any(axis=1)]
    if good.shape[0] < 2:
        raise ValueError("niqe_finish: %d of %d blocks have features without a NaN, the covariance needs 2"
                         % (good.shape[0], f.shape[0]))
    mu = np.nanmean(f, axis=0)
    cov = np.cov(good, rowvar=False)
    d = mu_p - mu
    return float(np.sqrt(d @ np.linalg.pinv((cov_p + cov) / 2.0) @ d))


def niqe(img, params, shave=0, block=96):
    """NIQE of one picture (lower is better): niqe_finish(niqe_features(img, shave, block), *params).  params: (mu_p,
    cov_p), what utils.load_niqe_params / utils.fit_niqe_params return.  Syncs (the finish is host arithmetic)."""
    mu_p, cov_p = params
    return niqe_finish(niqe_features(img, shave, block), mu_p, cov_p)


# ------------------------------------------------------------------------------------------------
# Raw video frames (YUV4MPEG2 payloads) to the net and back (csrc/video.hip): the front and the tail of test_video
# ------------------------------------------------------------------------------------------------
YUV_SUBSAMPLING = {"420": _lib.YUV_420, "444": _lib.YUV_444, "mono": _lib.YUV_MONO}


class YuvLayout(object):
    """Where the planes of one planar 8-bit frame lie: W, H, sub ('420', '444' or 'mono'), the chroma plane's size cw x
    ch (0 x 0 for mono), the byte offsets y_off / cb_off / cr_off inside the frame and frame_bytes.  Made by yuv_layout
    alone: the container (data.Y4MReader / Y4MWriter) and the kernels' launchers (yuv_unpack / yuv_pack) read the same
    object."""
    __slots__ = ("W", "H", "sub", "cw", "ch", "y_off", "cb_off", "cr_off", "frame_bytes")

    def __init__(self, W, H, sub, cw, ch):
        self.W, self.H, self.sub, self.cw, self.ch = W, H, sub, cw, ch
        self.y_off, self.cb_off, self.cr_off = 0, W * H, W * H + cw * ch
        self.frame_bytes = W * H + 2 * cw * ch

    @property
    def code(self):
        return YUV_SUBSAMPLING[self.sub]

    def scaled(self, W, H):
        """The layout of a W x H frame of the same subsampling (the output side of a stream)."""
        return yuv_layout(W, H, self.sub)

    def __eq__(self, other):
        return isinstance(other, YuvLayout) and (self.W, self.H, self.sub) == (other.W, other.H, other.sub)

    def __repr__(self):
        return "YuvLayout(%d x %d, %s, %d bytes)" % (self.W, self.H, self.sub, self.frame_bytes)


def yuv_layout(W, H, sub="420", tag=None):
    """The one derivation of a frame's layout.  Chroma planes of 4:2:0 are ceil(W/2) x ceil(H/2) by the format's
    definition; a 4:2:0 frame with an odd W or H is refused by name (`tag`: the stream's own C tag for the message)."""
    W, H = int(W), int(H)
    if sub not in YUV_SUBSAMPLING:
        raise ValueError("yuv_layout: subsampling must be '420', '444' or 'mono' (got %r)" % (sub,))
    if W <= 0 or H <= 0:
        raise ValueError("yuv_layout: a frame of %d x %d" % (W, H))
    if sub == "420" and (W % 2 or H % 2):
        raise ValueError("%s: a 4:2:0 frame of odd size W%d H%d is refused (its chroma planes would be ceil(W/2) x ceil(H/2) = "
                         "%d x %d; the 2 x 2 shrink of the output has no definition there)"
                         % (tag or "C420", W, H, (W + 1) // 2, (H + 1) // 2))
    cw, ch = {"420": ((W + 1) // 2, (H + 1) // 2), "444": (W, H), "mono": (0, 0)}[sub]
    return YuvLayout(W, H, sub, cw, ch)


def _yuv_frames(what, frames, layout, n=None):
    """frames: uint8 [N, >= frame_bytes] with dense bytes inside a frame (any frame stride, any first byte)."""
    if frames.dtype != torch.uint8 or frames.dim() != 2 or frames.shape[0] == 0 or frames.shape[1] < layout.frame_bytes \
            or frames.stride(1) != 1 or (frames.shape[0] > 1 and frames.stride(0) < layout.frame_bytes) \
            or (n is not None and frames.shape[0] != n):
        raise RuntimeError("%s: frames must be uint8 [%s, >= %d] with dense frames, got %s %s strides %s"
                           % (what, "N" if n is None else n, layout.frame_bytes, frames.dtype, tuple(frames.shape),
                              tuple(frames.stride())))
    return int(frames.shape[0]), (int(frames.stride(0)) if frames.shape[0] > 1 else max(int(frames.stride(0)), layout.frame_bytes))


def yuv_chroma(frames_u8, layout, oh, ow):
    """The chroma planes of N packed frames through srk_img_resize_u8 (bicubic, centre-aligned: C420jpeg's siting) to
    oh x ow: uint8 [2, N, oh, ow], all Cb planes then all Cr planes -- what yuv_unpack takes as chroma_full (oh x ow =
    H x W) and yuv_pack as chroma (the output frame's chroma size).  The 2 N planes go in two calls: inside a frame Cb
    and Cr lie cw * ch bytes apart, across frames frame_bytes, and the resizer takes one plane stride."""
    _require_u8("yuv_chroma", frames_u8)
    n, fs = _yuv_frames("yuv_chroma", frames_u8, layout)
    if layout.sub == "mono":
        raise RuntimeError("yuv_chroma: a mono stream has no chroma planes")
    out = torch.empty((2, n, int(oh), int(ow)), dtype=torch.uint8, device=frames_u8.device)
    for k, off in enumerate((layout.cb_off, layout.cr_off)):   # each call writes its half of the one buffer
        planes = torch.as_strided(frames_u8, (n, layout.ch, layout.cw), (fs, layout.cw, 1), frames_u8.storage_offset() + off)
        resize_u8(planes, int(oh), int(ow), out=out[k])
    return out


def yuv_unpack(frames_u8, layout, num_channels, chroma_full=None, out=None):
    """N packed frames (uint8 [N, frame_bytes], any frame stride, any first byte) -> the net's input, fp32 [N,C,H,W], one
    launch (k_yuv_unpack).  num_channels 1: Y / 255, the chroma is not read.  3: R, G, B / 255 through Pillow's YCbCr ->
    RGB tables from Y and full-resolution chroma: the frame's own (4:4:4), 128 (mono), or for 4:2:0 chroma_full
    ([2,N,H,W], None: yuv_chroma makes it here)."""
    _require_u8("yuv_unpack", frames_u8)
    n, fs = _yuv_frames("yuv_unpack", frames_u8, layout)
    c = int(num_channels)
    if c not in (1, 3):
        raise RuntimeError("yuv_unpack: num_channels must be 1 or 3 (got %d)" % c)
    if c == 3 and layout.sub == "420":
        if chroma_full is None:
            chroma_full = yuv_chroma(frames_u8, layout, layout.H, layout.W)
        _require_u8("yuv_unpack", chroma_full)
        if tuple(chroma_full.shape) != (2, n, layout.H, layout.W) or not chroma_full.is_contiguous():
            raise RuntimeError("yuv_unpack: chroma_full must be a dense uint8 [2,%d,%d,%d] tensor, got %s"
                               % (n, layout.H, layout.W, tuple(chroma_full.shape)))
    else:
        chroma_full = None
    out = _f32_out("yuv_unpack", (n, c, layout.H, layout.W), frames_u8.device, out)
    check(_lib.load().srk_yuv_unpack(ptr(frames_u8), fs, n, layout.H, layout.W, layout.code, c, ptr(chroma_full), ptr(out),
                                     stream_ptr()), "srk_yuv_unpack")
    return out


def yuv_pack(y, layout, chroma=None, out=None):
    """The net's output y (fp32 [N,C,OH,OW], any strides: a channels-last output is read in place) -> N packed frames of
    `layout` (the OUTPUT frame: layout.H x layout.W = OH x OW), uint8 [N, frame_bytes], one launch.  Quantised like
    to_u8_image.  C = 1: the Y' plane, and `chroma` (uint8 [2,N,ch,cw], yuv_chroma's; not for mono) copied into the Cb and
    Cr slots.  C = 3: Pillow's RGB -> YCbCr tables; 4:2:0 shrinks the chroma like Image.resize(..., Image.BOX)."""
    require_cuda(y)
    y = y.detach()
    if y.dim() != 4 or y.shape[1] not in (1, 3) or tuple(y.shape[2:]) != (layout.H, layout.W) or y.shape[0] == 0:
        raise RuntimeError("yuv_pack: expects a [N,C,%d,%d] tensor with C = 1 or 3, got %s" % (layout.H, layout.W, tuple(y.shape)))
    n, c = int(y.shape[0]), int(y.shape[1])
    if c == 1 and layout.sub != "mono":
        if chroma is None:
            raise RuntimeError("yuv_pack: a one-channel output on a %s stream needs the resized chroma planes" % layout.sub)
        _require_u8("yuv_pack", chroma)
        if tuple(chroma.shape) != (2, n, layout.ch, layout.cw) or not chroma.is_contiguous():
            raise RuntimeError("yuv_pack: chroma must be a dense uint8 [2,%d,%d,%d] tensor, got %s"
                               % (n, layout.ch, layout.cw, tuple(chroma.shape)))
    else:
        chroma = None
    if out is None:
        out = torch.empty((n, layout.frame_bytes), dtype=torch.uint8, device=y.device)
    _require_u8("yuv_pack", out)
    _, fs = _yuv_frames("yuv_pack: out", out, layout, n)
    check(_lib.load().srk_yuv_pack(ptr(y), _strides4(y), n, c, layout.H, layout.W, layout.code, ptr(chroma), ptr(out), fs,
                                   stream_ptr()), "srk_yuv_pack")
    return out


def _np_ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def yuv_unpack_host(frames_u8, layout, num_channels, chroma_full=None):
    """yuv_unpack on host memory (srk_yuv_unpack_host: the kernels' per-pixel header in plain C++): numpy uint8
    [N, frame_bytes] (any frame stride) -> numpy float32 [N,C,H,W].  chroma_full ([2,N,H,W]) is the caller's for 4:2:0
    with num_channels 3: there is no host resizer."""
    f = np.asarray(frames_u8)
    if f.dtype != np.uint8 or f.ndim != 2 or f.shape[1] < layout.frame_bytes or f.strides[1] != 1:
        raise ValueError("yuv_unpack_host: frames must be uint8 [N, >= %d] with dense frames" % layout.frame_bytes)
    n, c = int(f.shape[0]), int(num_channels)
    if chroma_full is not None:
        chroma_full = np.ascontiguousarray(chroma_full, dtype=np.uint8)
        if chroma_full.shape != (2, n, layout.H, layout.W):
            raise ValueError("yuv_unpack_host: chroma_full must be [2,%d,%d,%d]" % (n, layout.H, layout.W))
    out = np.empty((n, c, layout.H, layout.W), dtype=np.float32)
    check(_lib.load().srk_yuv_unpack_host(_np_ptr(f), int(f.strides[0]) if n > 1 else max(int(f.strides[0]), layout.frame_bytes),
                                          n, layout.H, layout.W, layout.code, c, _np_ptr(chroma_full), _np_ptr(out)),
          "srk_yuv_unpack_host")
    return out


def yuv_pack_host(y, layout, chroma=None):
    """yuv_pack on host memory (srk_yuv_pack_host): numpy float32 [N,C,OH,OW] of any strides -> numpy uint8
    [N, frame_bytes]."""
    y = np.asarray(y)
    if y.dtype != np.float32 or y.ndim != 4 or y.shape[2:] != (layout.H, layout.W) or any(s % 4 or s < 0 for s in y.strides):
        raise ValueError("yuv_pack_host: expects a float32 [N,C,%d,%d] array, got %s %s" % (layout.H, layout.W, y.dtype, y.shape))
    n, c = int(y.shape[0]), int(y.shape[1])
    if chroma is not None:
        chroma = np.ascontiguousarray(chroma, dtype=np.uint8)
        if chroma.shape != (2, n, layout.ch, layout.cw):
            raise ValueError("yuv_pack_host: chroma must be [2,%d,%d,%d]" % (n, layout.ch, layout.cw))
    out = np.zeros((n, layout.frame_bytes), dtype=np.uint8)
    strides = (ctypes.c_int64 * 4)(*[s // 4 for s in y.strides])
    check(_lib.load().srk_yuv_pack_host(_np_ptr(y), strides, n, c, layout.H, layout.W, layout.code, _np_ptr(chroma), _np_ptr(out),
                                        layout.frame_bytes), "srk_yuv_pack_host")
    return out
