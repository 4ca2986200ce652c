"""The yardstick of the LPIPS tests: the definition of DESIGN.md 27 restated with stock torch on the CPU -- one tapped
layer's distance, and the whole metric on torchvision's vgg16.features layout built from stock torch.nn layers with the
weights oracle.fill gives it -- in float64 (the reference) and float32 (torch's own fp32 evaluation of the same graph),
plus the case tables and the bars the tests hold the host twin and the device path to.

The norm is torch.linalg.vector_norm, whose subgradient at an all-zero pixel is 0: the rule the kernels follow (plain
sqrt(sum(f^2)) autograd gives NaN there, and a ReLU map has such pixels).

Bars.  The project's contract is 1e-4 * max|ref| for values and 1e-3 * max|ref| for gradients.  The layer op is fp64
inside and meets that plainly.  The whole net runs through ReLU and pool decisions that any fp32 evaluation can flip, so
for it perceptual_ref.bar's rule applies: the contract, or twice the error of torch's own fp32 CPU evaluation against
fp64 on the same inputs, whichever is larger.  Both numbers are printed by the tests and recorded in
profiles/lpips_parity.txt."""
import copy
import functools
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fill  # noqa: E402
from perceptual_ref import bar, max_err  # noqa: E402,F401  (the one rule for a bar through fp32 ReLU / pool decisions)

VGG16_CFG = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512)
TAPS = (3, 8, 15, 22, 29)
WIDTHS = (64, 128, 256, 512, 512)
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
EPS = 1e-10
OUT_CONTRACT, GRAD_CONTRACT = 1e-4, 1e-3

# [N, H, W, C] as the kernels see them (the tensors are [N, C, H, W]); C = 3 and 70 take the 4-byte path with a ragged
# lane tail, 64 / 128 / 256 / 512 the four lane groupings of the 16-byte path, (1, 9, 8, 64) more than one block a sample
LAYER_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 3), (1, 4, 4, 64), (2, 5, 7, 70), (1, 2, 3, 128), (3, 1, 9, 256), (1, 3, 3, 512),
                (1, 9, 8, 64)]
# whole metric: the smallest inputs that reach 1 x 1 at the fifth tap, odd sizes at every pool
METRIC_SHAPES = [(2, 3, 16, 16), (1, 3, 17, 19), (1, 3, 32, 24)]


# -- one layer --------------------------------------------------------------------------------------------------------
def layer_values(f0, f1, w):
    """value[n] = mean_hw sum_c w[c] (f0 / (||f0|| + eps) - f1 / (||f1|| + eps))^2 of [N,C,H,W] maps, in their dtype."""
    a = torch.linalg.vector_norm(f0, dim=1, keepdim=True) + EPS
    b = torch.linalg.vector_norm(f1, dim=1, keepdim=True) + EPS
    q = f0 / a - f1 / b
    return (w.view(1, -1, 1, 1) * q * q).sum(1).mean((1, 2))


@functools.lru_cache(maxsize=None)
def layer_case(shape):
    """Inputs and the fp64 results of one layer case: f0, f1 [N,C,H,W] fp32 = relu(randn) with all-zero pixels planted in
    f0 only, in f1 only and in both (where the case has three pixels), w >= 0, the upstream g [N] fp64; value [N] and
    df0 in fp64."""
    n, h, w_, c = shape
    seed = 900 + 7 * n + 11 * h + 13 * w_ + c
    f0, f1 = torch.relu(fill.randn((n, c, h, w_), seed)), torch.relu(fill.randn((n, c, h, w_), seed + 1))
    if n * h * w_ >= 3:
        flat0, flat1 = f0.permute(0, 2, 3, 1).reshape(-1, c), f1.permute(0, 2, 3, 1).reshape(-1, c)
        last = n * h * w_ - 1
        z0, z1 = torch.ones(n * h * w_), torch.ones(n * h * w_)
        z0[0] = z0[last] = 0.0        # pixel 0: f0 only; the last pixel: both
        z1[1] = z1[last] = 0.0        # pixel 1: f1 only
        f0 = (flat0 * z0[:, None]).reshape(n, h, w_, c).permute(0, 3, 1, 2).contiguous()
        f1 = (flat1 * z1[:, None]).reshape(n, h, w_, c).permute(0, 3, 1, 2).contiguous()
    w = fill.rand((c,), seed + 2)
    g = fill.randn((n,), seed + 3).double()
    x = f0.double().requires_grad_(True)
    value = layer_values(x, f1.double(), w.double())
    (value * g).sum().backward()
    assert bool(torch.isfinite(x.grad).all())
    return {"f0": f0, "f1": f1, "w": w, "g": g, "value": value.detach(), "df0": x.grad.detach()}


def host_layer(lib, f0, f1, w, g=None):
    """srk_lpips_layer_host on [N,C,H,W] fp32 tensors: (value [N], df0 [N,C,H,W] or None), float64."""
    import ctypes
    n, c, h, w_ = f0.shape
    a = f0.permute(0, 2, 3, 1).contiguous()
    b = f1.permute(0, 2, 3, 1).contiguous()
    wc = w.contiguous()
    value = torch.empty(n, dtype=torch.float64)
    df0 = torch.empty((n, h, w_, c), dtype=torch.float64) if g is not None else None
    gc = g.double().contiguous() if g is not None else None
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = lib.srk_lpips_layer_host(p(a), p(b), p(wc), p(gc), n, h, w_, c, p(value), p(df0))
    assert rc == 0, (rc, lib.srk_last_error_string())
    return value, (df0.permute(0, 3, 1, 2) if df0 is not None else None)


# -- the whole metric ---------------------------------------------------------------------------------------------------
def torch_vgg16():
    """vgg16.features[:30] from stock torch.nn layers (what torchvision constructs), float32."""
    mods, cin = [], 3
    for v in VGG16_CFG:
        if v == 'M':
            mods.append(nn.MaxPool2d(2, 2))
        else:
            mods += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(False)]
            cin = v
    return nn.Sequential(*mods)


@functools.lru_cache(maxsize=None)
def filled_net(seed=91):
    """(float32 features, their float64 copy, lins [five float32 vectors >= 0], the vgg16 state_dict under torchvision's
    names, the lins state_dict under the `lpips` package's names)."""
    f32 = fill.fill_module(torch_vgg16(), seed)
    f64 = copy.deepcopy(f32).double()
    for p in list(f32.parameters()) + list(f64.parameters()):
        p.requires_grad_(False)
    lins = [fill.rand((c,), seed + 1 + l) for l, c in enumerate(WIDTHS)]
    vgg_sd = {"features." + k: v.clone() for k, v in f32.state_dict().items()}
    vgg_sd["classifier.0.weight"] = torch.zeros(2, 2)     # (a real file holds more than the features)
    lin_sd = {"lin%d.model.1.weight" % l: v.clone().view(1, -1, 1, 1) for l, v in enumerate(lins)}
    return f32, f64, lins, vgg_sd, lin_sd


def scale_input(x, normalize):
    s = torch.tensor(SHIFT, dtype=x.dtype).view(-1, 1, 1)
    d = torch.tensor(SCALE, dtype=x.dtype).view(-1, 1, 1)
    return ((2 * x - 1 if normalize else x) - s) / d


def taps(features, x):
    out = []
    for i, m in enumerate(features):
        x = m(x)
        if i in TAPS:
            out.append(x)
    return out


def lpips_torch(features, lins, pred, target, normalize=True):
    """The per-sample LPIPS values [N], differentiable in pred, in the dtype of `features`; the target side is detached."""
    dt = next(features.parameters()).dtype
    with torch.no_grad():
        real = taps(features, scale_input(target.detach().to(dt), normalize))
    fake = taps(features, scale_input(pred.to(dt), normalize))
    return sum(layer_values(a, b, w.to(dt)) for a, b, w in zip(fake, real, lins))


def metric_eval(features, lins, pred, target, normalize):
    """(values [N], d mean(values) / d pred) in the dtype of `features`."""
    p = pred.detach().to(next(features.parameters()).dtype).requires_grad_(True)
    v = lpips_torch(features, lins, p, target, normalize)
    v.mean().backward()
    return v.detach(), p.grad.detach()


@functools.lru_cache(maxsize=None)
def metric_case(shape, normalize):
    """Inputs and the fp64 / fp32-CPU results of one whole-metric case, computed once."""
    f32, f64, lins, _, _ = filled_net()
    lo, hi = (0.0, 1.0) if normalize else (-1.0, 1.0)
    pred, target = fill.rand(shape, 940 + shape[2], lo, hi), fill.rand(shape, 950 + shape[3], lo, hi)
    v64, d64 = metric_eval(f64, lins, pred, target, normalize)
    v32, d32 = metric_eval(f32, lins, pred, target, normalize)
    return {"pred": pred, "target": target, "v64": v64, "d64": d64, "v_err32": max_err(v32, v64)[0],
            "d_err32": max_err(d32, d64)[0]}
