"""The fp64 restatement of the channel-slice convolution, the residual dense block and RDN: plain torch.cat + F.conv2d in
double.  Everything the dense tests compare against comes from here; nothing in it touches the package's kernels.

Layout helpers: the kernels work on channel SLICES of wider NHWC buffers; `Buf` makes such a buffer (optionally NaN
outside the slice), hands out the slice as an NCHW double tensor for the restatement and as a pointer + stride for the
host twin (srk_dense_conv_host) or a device tensor + channel offset for ops.dense_conv."""
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 3
SLOPE = 0.2


def worst(got, want):
    """max |got - want| / max |want| (1 where the reference is all zero)."""
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def rand(shape, seed, std=1.0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((std * rs.standard_normal(shape)).astype(np.float32))


# ---- one convolution -----------------------------------------------------------------------------------------------------
def act64(v, act, slope=SLOPE):
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_LRELU:
        return F.leaky_relu(v, slope)
    return v


def conv_forward(a, b, w, bias, act=ACT_NONE, slope=SLOPE, residual=None):
    """a [N, CA, H, W], b [N, CB, H, W] or None, w [Cout, CA + CB, K, K]: everything is taken to double."""
    x = a.double() if b is None else torch.cat((a.double(), b.double()), 1)
    y = act64(F.conv2d(x, w.double(), None if bias is None else bias.double(), padding=w.shape[-1] // 2), act, slope)
    return y if residual is None else y + residual.double()


def conv_grads(a, b, w, bias, dy, act=ACT_NONE, slope=SLOPE):
    """(y, da, db, dw, dbias) of sum(y * dy) through autograd, in double; the residual has no part in these."""
    a64 = a.double().requires_grad_(True)
    b64 = None if b is None else b.double().requires_grad_(True)
    w64, bias64 = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    y = conv_forward(a64, b64, w64, bias64, act, slope)
    (y * dy.double()).sum().backward()
    return y.detach(), a64.grad, (None if b is None else b64.grad), w64.grad, bias64.grad


class Buf(object):
    """A dense NHWC fp32 buffer [N, H, W, width] holding a slice of `c` channels from channel `off`.  The slice is filled
    from `seed` (or zeros / NaN); the rest of the buffer holds `outside` (NaN to prove it is never read, or a pattern to
    prove it is never written)."""

    def __init__(self, n, h, w, c, off=0, width=None, seed=None, outside=float("nan"), inside=None, std=1.0):
        width = off + c if width is None else width
        assert off + c <= width
        self.n, self.h, self.w, self.c, self.off, self.width = n, h, w, c, off, width
        self.t = torch.full((n, h, w, width), outside, dtype=torch.float32)
        if seed is not None:
            self.t[..., off:off + c] = rand((n, h, w, c), seed, std)
        elif inside is not None:
            self.t[..., off:off + c] = inside

    def nchw(self):
        """the slice as an NCHW tensor (a copy)"""
        return self.t[..., self.off:self.off + self.c].permute(0, 3, 1, 2).contiguous()

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * self.off)

    def device(self, dev):
        """[N, width, H, W] channels_last on the device (the same memory layout)"""
        return self.t.to(dev).permute(0, 3, 1, 2)

    def outside_equal(self, other_nhwc):
        """every element outside the slice has the bits it started with"""
        mask = torch.ones(self.width, dtype=torch.bool)
        mask[self.off:self.off + self.c] = False
        a = self.t[..., mask].view(torch.int32)
        b = other_nhwc.cpu()[..., mask].contiguous().view(torch.int32)
        return bool(torch.equal(a, b))


def from_device(t_nchw_cl):
    """a channels_last device tensor -> NHWC host tensor"""
    return t_nchw_cl.detach().permute(0, 2, 3, 1).contiguous().cpu()


def desc(pkg, n, h, w, k, ca, cb, cout, act=ACT_NONE, slope=SLOPE, terms=3, **ld):
    d = pkg._lib.DenseDesc()
    d.N, d.H, d.W, d.K, d.CA, d.CB, d.Cout = n, h, w, k, ca, cb, cout
    d.act, d.slope, d.terms = act, slope, terms
    for name, v in ld.items():
        setattr(d, name, v)
    return d


def fptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- the block, the trunk, the net ----------------------------------------------------------------------------------------
def rdb_forward(x, params):
    """One residual dense block in whatever dtype x and params have: params = (w_1, b_1, ..., w_C, b_C, w_lff, b_lff)."""
    C = len(params) // 2 - 1
    feats = x
    for c in range(C):
        feats = torch.cat((feats, torch.relu(F.conv2d(feats, params[2 * c], params[2 * c + 1], padding=1))), 1)
    return F.conv2d(feats, params[2 * C], params[2 * C + 1]) + x


def trunk_forward(x, blocks):
    """cat(RDB_1 .. RDB_D outputs): what ops.residual_dense_blocks returns."""
    outs = []
    for p in blocks:
        x = rdb_forward(x, p)
        outs.append(x)
    return torch.cat(outs, 1)


def make_blocks(g0, g, C, D, seed, gain=0.7):
    blocks = []
    for d in range(D):
        p = []
        for c in range(C + 1):
            cin, cout, k = (g0 + c * g, g, 3) if c < C else (g0 + C * g, g0, 1)
            p.append(rand((cout, cin, k, k), seed + 100 * d + 2 * c, gain * (2.0 / (cin * k * k)) ** 0.5))
            p.append(rand((cout,), seed + 100 * d + 2 * c + 1, 0.05))
        blocks.append(tuple(p))
    return blocks


class _RefRDBConv(nn.Module):
    def __init__(self, cin, g):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(cin, g, 3, padding=1), nn.ReLU())

    def forward(self, x):
        return torch.cat((x, self.conv(x)), 1)


class _RefRDB(nn.Module):
    def __init__(self, g0, g, C):
        super().__init__()
        self.convs = nn.Sequential(*[_RefRDBConv(g0 + c * g, g) for c in range(C)])
        self.LFF = nn.Conv2d(g0 + C * g, g0, 1)

    def forward(self, x):
        return self.LFF(self.convs(x)) + x


class RefRDN(nn.Module):
    """RDN in plain torch with the official module names; loads the package's state_dict."""

    def __init__(self, num_channels, G0=64, D=16, C=8, G=64, scale_factor=4):
        super().__init__()
        self.SFENet1 = nn.Conv2d(num_channels, G0, 3, padding=1)
        self.SFENet2 = nn.Conv2d(G0, G0, 3, padding=1)
        self.RDBs = nn.ModuleList([_RefRDB(G0, G, C) for _ in range(D)])
        self.GFF = nn.Sequential(nn.Conv2d(D * G0, G0, 1), nn.Conv2d(G0, G0, 3, padding=1))
        r = scale_factor
        if r == 4:
            up = [nn.Conv2d(G0, G * 4, 3, padding=1), nn.PixelShuffle(2), nn.Conv2d(G, G * 4, 3, padding=1), nn.PixelShuffle(2)]
        else:
            up = [nn.Conv2d(G0, G * r * r, 3, padding=1), nn.PixelShuffle(r)]
        self.UPNet = nn.Sequential(*(up + [nn.Conv2d(G, num_channels, 3, padding=1)]))

    def forward(self, x):
        f1 = self.SFENet1(x)
        x = self.SFENet2(f1)
        outs = []
        for b in self.RDBs:
            x = b(x)
            outs.append(x)
        return self.UPNet(self.GFF(torch.cat(outs, 1)) + f1)


def ref_rdn_like(net, *ctor):
    """The fp64 RefRDN carrying the parameters of the package's net."""
    ref = RefRDN(*ctor).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    return ref


def param_count(num_channels, G0, D, C, G, r):
    conv = lambda cin, cout, k: cout * cin * k * k + cout
    n = conv(num_channels, G0, 3) + conv(G0, G0, 3)
    n += D * (sum(conv(G0 + c * G, G, 3) for c in range(C)) + conv(G0 + C * G, G0, 1))
    n += conv(D * G0, G0, 1) + conv(G0, G0, 3)
    n += (conv(G0, 4 * G, 3) + conv(G, 4 * G, 3)) if r == 4 else conv(G0, G * r * r, 3)
    return n + conv(G, num_channels, 3)


# ---- the case table of the raw operator (tests/test_dense_cpu.py, tests/test_dense_conv_gpu.py) -----------------------------
# name -> (H, W, K, CA, CB, Cout, act, residual, terms).  N = 2 throughout.  No H x W is a multiple of the 16-pixel tile; every
# K, CA in {16, 64}, CB in {0, 16, 48, 160}, Cout in {16, 32, 64} (and 48), activation, residual and term count appears, and
# the two last cases are the smallest pictures at which the planner hands a wave 2 and 4 pixel tiles (N H W / 32 and
# N H W / 64 reach 1024), which the smaller ones never do.
CASES = {
    "1x1_k1": (1, 1, 1, 16, 0, 16, ACT_NONE, False, 3),
    "1x1_k3_two": (1, 1, 3, 16, 16, 32, ACT_RELU, True, 6),
    "3x5_single": (3, 5, 3, 16, 0, 16, ACT_RELU, False, 3),
    "3x5_k1_wide": (3, 5, 1, 64, 48, 64, ACT_NONE, True, 6),
    "3x5_b160": (3, 5, 3, 64, 160, 32, ACT_LRELU, False, 3),
    "7x9_b48": (7, 9, 3, 16, 48, 64, ACT_RELU, False, 6),
    "7x9_k1_lff": (7, 9, 1, 64, 160, 64, ACT_NONE, True, 3),
    "7x9_lrelu_res": (7, 9, 3, 64, 16, 16, ACT_LRELU, True, 6),
    "7x9_rdn_layer": (7, 9, 3, 64, 64, 32, ACT_RELU, False, 3),
    "17x33_big_k": (17, 33, 3, 64, 160, 64, ACT_RELU, False, 3),
    "17x33_k1_lrelu": (17, 33, 1, 16, 16, 32, ACT_LRELU, True, 3),
    "17x33_single_res": (17, 33, 3, 64, 0, 64, ACT_NONE, True, 6),
    "17x33_cout48": (17, 33, 3, 16, 48, 48, ACT_RELU, False, 6),
    "129x128_two_tiles": (129, 128, 3, 16, 16, 16, ACT_RELU, False, 3),
    "181x183_four_tiles": (181, 183, 3, 16, 16, 16, ACT_NONE, True, 6),
}
SMALL_CASES = [k for k, v in CASES.items() if v[0] * v[1] < 10000]
N = 2
_MADE = {}


class Case(object):
    """Buffers (slices at non-zero channel offsets of wider buffers, NaN around every source slice) and the fp64 results of
    one row of CASES.  Built once per process and shared; nobody writes into its members (destinations are cloned)."""

    def __init__(self, name):
        h, w, k, ca, cb, cout, act, res, terms = CASES[name]
        self.name, self.dims, self.k, self.act, self.terms = name, (N, h, w), k, act, terms
        self.ca, self.cb, self.cout, self.has_res = ca, cb, cout, res
        seed = 1000 + 37 * sorted(CASES).index(name)
        self.A = Buf(N, h, w, ca, off=16, width=ca + 48, seed=seed)
        self.B = Buf(N, h, w, cb, off=32, width=cb + 32 + 16, seed=seed + 1) if cb else None
        ctot = ca + cb
        self.W = rand((cout, ctot, k, k), seed + 2, (2.0 / (ctot * k * k)) ** 0.5)
        self.bias = rand((cout,), seed + 3, 0.1)
        self.R = Buf(N, h, w, cout, off=16, width=cout + 16, seed=seed + 4) if res else None
        self.DY = Buf(N, h, w, cout, off=48, width=cout + 64, seed=seed + 5)
        self.ADD = Buf(N, h, w, ca, off=16, width=ca + 32, seed=seed + 6)
        a, b = self.A.nchw(), (self.B.nchw() if cb else None)
        # the saved output of the backward is the activation's own output (the residual comes after it)
        self.y_act, self.da, self.db, self.dw, self.dbias = conv_grads(a, b, self.W, self.bias, self.DY.nchw(), act)
        self.y = self.y_act if not res else self.y_act + self.R.nchw().double()
        self.YS = Buf(N, h, w, cout, off=16, width=cout + 32, inside=self.y_act.permute(0, 2, 3, 1).float())

    def out_buf(self, c, off, width, inside=float("nan")):
        """a destination: a recognisable pattern outside the slice, `inside` (NaN: beta 0 must not read it) in it"""
        n, h, w = self.dims
        b = Buf(n, h, w, c, off=off, width=width, outside=0.0, inside=inside)
        pattern = torch.arange(b.t.numel(), dtype=torch.float32).view(b.t.shape) * 0.5 + 1.0
        keep = b.t[..., off:off + c].clone()
        b.t.copy_(pattern)
        b.t[..., off:off + c] = keep
        return b


def case(name):
    if name not in _MADE:
        _MADE[name] = Case(name)
    return _MADE[name]


def nhwc(t_nchw):
    return t_nchw.permute(0, 2, 3, 1)
