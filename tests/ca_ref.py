"""References for channel attention and RCAN (no GPU, no package code in the arithmetic):

  restate(...)        the operator of include/srk.h written out in fp64 torch, forward and the backward formulas one by one
  autograd(...)       fp64 torch autograd of the plain composition (adaptive_avg_pool2d, two conv2d, relu, sigmoid, mul, add);
                      restate is checked against it once (tests/test_ca_cpu.py)
  RefRCAN             a plain-torch RCAN that takes the package's state_dict, run in fp64
  cases()/make(...)   the case table of the issue and its seeded inputs
  host(...)           srk_channel_attention_host on numpy arrays
"""
import collections
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

# (N, C, Cr, H, W)
TABLE = collections.OrderedDict([
    ("hw1", (1, 4, 1, 1, 1)),            # HW = 1: the pool is the input
    ("cr1", (2, 16, 1, 3, 5)),           # Cr = 1
    ("scalar", (3, 6, 2, 7, 9)),         # C % 4 != 0: the scalar path; odd N
    ("net_odd", (2, 64, 4, 17, 23)),     # the net's channels, odd extents
    ("mid", (5, 32, 8, 8, 8)),
    ("wide", (1, 64, 4, 96, 100)),       # several partials a sample, up to the planner's cap
    ("patch", (2, 64, 4, 40, 40)),
    ("saturated", (2, 8, 2, 5, 6)),      # b2 = +40 / -40: s is 1 or ~4e-18
    ("dead_hidden", (2, 8, 2, 5, 6)),    # b1 = -1e3: h = 0
])
Case = collections.namedtuple("Case", "t x w1 b1 w2 b2 g")   # fp32 tensors, NCHW; x may be None
Result = collections.namedtuple("Result", "y dt dw1 db1 dw2 db2 s h")   # fp64


def cases():
    return list(TABLE)


def make(name, skip):
    """Seeded normals; parameters of std 0.5 (1x1 conv shapes)."""
    n, c, cr, h, w = TABLE[name]
    gen = torch.Generator().manual_seed(1000 + 2 * list(TABLE).index(name) + int(skip))
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    t, x, g = rn(n, c, h, w), (rn(n, c, h, w) if skip else None), rn(n, c, h, w)
    w1, b1, w2, b2 = 0.5 * rn(cr, c, 1, 1), 0.5 * rn(cr), 0.5 * rn(c, cr, 1, 1), 0.5 * rn(c)
    if name == "saturated":
        b2 = torch.where(torch.arange(c) < c // 2, torch.tensor(40.0), torch.tensor(-40.0))
    if name == "dead_hidden":
        b1 = torch.full((cr,), -1e3)
    return Case(t, x, w1, b1, w2, b2, g)


def restate(case):
    """The definition, every step written out, in fp64."""
    t, g = case.t.double(), case.g.double()
    w1, w2 = case.w1.double().flatten(1), case.w2.double().flatten(1)     # [Cr, C], [C, Cr]
    b1, b2 = case.b1.double(), case.b2.double()
    n, c, hh, ww = t.shape
    hw = hh * ww
    m = t.sum(dim=(2, 3)) / hw                                # [N, C]
    h = torch.clamp(m @ w1.t() + b1, min=0.0)                 # [N, Cr]
    s = 1.0 / (1.0 + torch.exp(-(h @ w2.t() + b2)))           # [N, C]
    y = t * s[:, :, None, None]
    if case.x is not None:
        y = y + case.x.double()
    ds = (g * t).sum(dim=(2, 3))
    da = ds * s * (1.0 - s)
    dh = (da @ w2) * (h > 0)
    dm = dh @ w1
    dt = g * s[:, :, None, None] + dm[:, :, None, None] / hw
    dw2, db2 = da.t() @ h, da.sum(0)
    dw1, db1 = dh.t() @ m, dh.sum(0)
    return Result(y, dt, dw1.reshape(case.w1.shape), db1, dw2.reshape(case.w2.shape), db2, s, h)


def composition(t, x, w1, b1, w2, b2):
    """The plain torch composition (any dtype, any device)."""
    s = torch.sigmoid(F.conv2d(F.relu(F.conv2d(F.adaptive_avg_pool2d(t, 1), w1, b1)), w2, b2))
    y = t * s
    return y + x if x is not None else y


def autograd(case):
    """fp64 torch autograd of the composition -> (y, dt, dx or None, dw1, db1, dw2, db2)."""
    leaves = [None if v is None else v.double().requires_grad_(True) for v in case[:6]]
    y = composition(*leaves)
    y.backward(case.g.double())
    gr = [None if v is None else v.grad for v in leaves]
    return (y.detach(), gr[0], gr[1]) + tuple(gr[2:])


def host(lib, case, backward=True):
    """srk_channel_attention_host -> Result of fp64 tensors in the case's NCHW shapes (s, h: None)."""
    n, c, hh, ww = case.t.shape
    cr = case.w1.shape[0]
    nhwc = lambda v: None if v is None else np.ascontiguousarray(v.numpy().transpose(0, 2, 3, 1))
    t, x, g = nhwc(case.t), nhwc(case.x), nhwc(case.g)
    par = [np.ascontiguousarray(v.numpy()).reshape(-1) for v in (case.w1, case.b1, case.w2, case.b2)]
    outs = [np.full(shape, np.nan, np.float64) for shape in
            ((n, hh, ww, c), (n, hh, ww, c), (cr, c), (cr,), (c, cr), (c,))]
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    rc = lib.srk_channel_attention_host(p(t), p(x), p(par[0]), p(par[1]), p(par[2]), p(par[3]), p(g) if backward else None,
                                        n, hh, ww, c, cr, *[p(o) if (backward or i == 0) else None for i, o in enumerate(outs)])
    assert rc == 0, lib.srk_last_error_string()
    y, dt = (torch.from_numpy(o.transpose(0, 3, 1, 2).copy()) for o in outs[:2])
    dw1, db1, dw2, db2 = (torch.from_numpy(o) for o in outs[2:])
    return Result(y, dt, dw1.reshape(case.w1.shape), db1, dw2.reshape(case.w2.shape), db2, None, None)


def worst(got, want):
    """max |got - want| / max |want| (1 where the reference is all zero)."""
    want = want.double()
    return float((got.double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-300)


# ---- RCAN in plain torch ------------------------------------------------------------------------------------------------
class _CA(nn.Module):
    def __init__(self, c, r):
        super().__init__()
        self.conv_du = nn.Sequential(nn.Conv2d(c, c // r, 1), nn.ReLU(), nn.Conv2d(c // r, c, 1), nn.Sigmoid())

    def forward(self, t):
        return t * self.conv_du(F.adaptive_avg_pool2d(t, 1))


class _RCAB(nn.Module):
    def __init__(self, c, r):
        super().__init__()
        self.conv1, self.conv2, self.ca = nn.Conv2d(c, c, 3, 1, 1), nn.Conv2d(c, c, 3, 1, 1), _CA(c, r)

    def forward(self, x):
        return x + self.ca(self.conv2(F.relu(self.conv1(x))))


class _Wrapped(nn.Module):
    """A conv under the attribute name the package's blocks give it (`conv`)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, 1, 1)

    def forward(self, x):
        return self.conv(x)


class _Group(nn.Module):
    def __init__(self, c, blocks, r):
        super().__init__()
        self.blocks = nn.Sequential(*[_RCAB(c, r) for _ in range(blocks)])
        self.conv = _Wrapped(c, c)

    def forward(self, x):
        return x + self.conv(self.blocks(x))


class _Up(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.upsample = _Wrapped(c, 4 * c)

    def forward(self, x):
        return F.pixel_shuffle(self.upsample(x), 2)


class RefRCAN(nn.Module):
    def __init__(self, num_channels, base_filter, num_groups, num_blocks, reduction, scale_factor):
        super().__init__()
        self.input_conv = _Wrapped(num_channels, base_filter)
        self.residual_groups = nn.Sequential(*[_Group(base_filter, num_blocks, reduction) for _ in range(num_groups)])
        self.mid_conv = _Wrapped(base_filter, base_filter)
        self.upscale = nn.Sequential(*[_Up(base_filter) for _ in range({2: 1, 4: 2, 8: 3}[scale_factor])])
        self.output_conv = _Wrapped(base_filter, num_channels)

    def forward(self, x):
        head = self.input_conv(x)
        return self.output_conv(self.upscale(head + self.mid_conv(self.residual_groups(head))))


def ref_rcan_like(net, *ctor):
    """RefRCAN(*ctor) in fp64 with the package net's weights."""
    ref = RefRCAN(*ctor).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    return ref
