"""What tests/test_fft_loss_cpu.py and tests/test_fft_loss_gpu.py share: the frequency-domain loss restated in fp64 numpy
and torch on the CPU, and the case table.

    F = s * W_H d W_W^T,  loss = sum(|Re F| + |Im F|) / (2 M),  G = sign(Re F) + i sign(Im F),
    d loss / d pred = s / (2 M) * Re(conj(W_H) G conj(W_W)^T)

with W_n[u, y] = cos - i sin of the library's own table at index (u * y) mod n.  The table (srk_dft_table_host) is the
only thing taken from the package under test: the twiddles are data, so that Im F is an exact zero at the self-conjugate
bins for the kernels, the host twin and this restatement alike.  Real and imaginary parts are kept as separate real
matrix products (no complex BLAS), so those zeros are exact here too."""
import ctypes
import functools

import numpy as np
import torch

SEED = 1234
MAX_DIM = 256
DEVICE_ONLY = ("many_items",)    # cases about the kernels' grids: the host twin (a plain loop, 24 s on this one) skips them

# the issue's table.  The kernels' work items are 128 rows or columns (lane l owns entries l and l + 64, indexed across
# planes) times 4 outputs; k_fft_diff moves 16 x 16 tiles.  12 straddles all of them: its 2 x 34 half-spectrum columns put
# the plane boundary inside one lane set and four columns into the second set; its 260 rows are two full items with the
# plane boundary inside the second and a third of four rows; 130 = 32 * 4 + 2, 34 = 8 * 4 + 2 and 66 = 16 * 4 + 2 leave
# a ragged last group of outputs on every axis, 130 and 66 a ragged tile both ways.  13 has 129 columns: a second item of
# one column.  "many_items" (below) has more items than a launch has waves, so a wave takes several.
SHAPES = [(1, 1, 1, 1), (1, 1, 1, 7), (2, 1, 2, 2), (1, 3, 8, 8), (2, 3, 7, 5), (1, 1, 6, 10), (2, 5, 16, 16),
          (1, 3, 17, 33), (2, 1, 41, 41), (1, 3, 48, 64), (1, 1, 128, 128), (1, 2, 130, 66), (1, 1, 256, 256),
          (1, 1, 256, 3)]


@functools.lru_cache(maxsize=None)
def _lib():
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    return p._lib.load()


@functools.lru_cache(maxsize=None)
def table(n):
    """srk_dft_table_host(n) as an [n, 2] fp64 array of (cos, sin)(2 pi k / n)."""
    out = np.full((n, 2), np.nan, np.float64)
    rc = _lib().srk_dft_table_host(n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == 0
    return out


@functools.lru_cache(maxsize=None)
def dft_matrices(n):
    """(C, S): C[u, y] = cos(2 pi u y / n), S[u, y] = sin(...), entries of the table at (u * y) mod n."""
    k = np.arange(n, dtype=np.int64)
    idx = (k[:, None] * k[None, :]) % n
    t = table(n)
    return t[idx, 0].copy(), t[idx, 1].copy()


def norm_scale(norm, h, w):
    return {"backward": 1.0, "ortho": 1.0 / np.sqrt(float(h) * float(w))}[norm]


def spectrum(d, norm="backward"):
    """(Re F, Im F) of fp64 [..., H, W]."""
    h, w = d.shape[-2:]
    ch, sh = dft_matrices(h)
    cw, sw = dft_matrices(w)
    tre, tim = d @ cw.T, -(d @ sw.T)
    s = norm_scale(norm, h, w)
    return s * (ch @ tre + sh @ tim), s * (ch @ tim - sh @ tre)


def structural_zero(h, w):
    """[H, W] bool: the bins whose Im F is an exact zero for any real plane (2u = 0 mod H and 2v = 0 mod W)."""
    u, v = np.arange(h)[:, None], np.arange(w)[None, :]
    return ((2 * u) % h == 0) & ((2 * v) % w == 0)


def loss_and_grad(pred, gt, norm="backward"):
    """(loss, d loss / d pred) of fp32 [N,C,H,W] arrays in closed form, fp64."""
    d = np.asarray(pred, np.float64) - np.asarray(gt, np.float64)
    h, w = d.shape[-2:]
    fre, fim = spectrum(d, norm)
    loss = (np.abs(fre) + np.abs(fim)).sum() / (2.0 * d.size)
    gr, gi = np.sign(fre), np.sign(fim)          # sign(0) = 0; a NaN stays a NaN
    ch, sh = dft_matrices(h)
    cw, sw = dft_matrices(w)
    sre, sim = ch @ gr - sh @ gi, sh @ gr + ch @ gi
    grad = norm_scale(norm, h, w) / (2.0 * d.size) * (sre @ cw.T - sim @ sw.T)
    return float(loss), grad


def torch_loss(x, y, norm="backward"):
    """The same loss on fp64 torch tensors through the same matrices, for autograd (CPU oracle steps, the gradient's
    cross-check)."""
    d = x - y
    h, w = d.shape[-2:]
    ch, sh = (torch.from_numpy(m) for m in dft_matrices(h))
    cw, sw = (torch.from_numpy(m) for m in dft_matrices(w))
    tre, tim = d @ cw.T, -(d @ sw.T)
    fre, fim = ch @ tre + sh @ tim, ch @ tim - sh @ tre
    return norm_scale(norm, h, w) * (fre.abs() + fim.abs()).sum() / (2.0 * d.numel())


def mix_loss(pixel, w, norm="backward"):
    """pixel(pred, t) + w * FFT(pred, t) for torch tensors of any float dtype."""
    def loss(pred, t):
        return pixel(pred, t) + w * torch_loss(pred.double(), t.double(), norm).to(pred.dtype)
    return loss


def _pair(shape, seed=SEED):
    rng = np.random.RandomState(seed)
    g = rng.rand(*shape).astype(np.float32)
    p = (g + 0.1 * rng.randn(*shape)).astype(np.float32)
    return p, g


@functools.lru_cache(maxsize=None)
def _table():
    out = {}
    for i, shape in enumerate(SHAPES):
        out["%02d_%s" % (i + 1, "x".join(str(v) for v in shape))] = _pair(shape) + ("backward",)
    g = _pair((2, 3, 16, 12))[1]
    out["identical"] = (g.copy(), g, "backward")
    p, g = _pair((1, 3, 12, 20))
    p = p.copy()
    p[:, :, ::3, ::4] += 2.5          # far outside [0, 1], both ways: nothing clamps the prediction
    p[:, :, 1::3, 1::4] -= 3.0
    out["out_of_range"] = (p, g, "backward")
    out["ortho"] = _pair((2, 3, 16, 24)) + ("ortho",)
    # 17,550 columns = 138 items x 32 groups of rows = 4,416 wave items for the 4,096 waves of a column-pass launch (and 4,590
    # for the row passes): the grid-stride path of every kernel
    out["many_items"] = _pair((90, 3, 128, 128)) + ("backward",)
    return out


def cases():
    """name -> (pred, gt, norm), fp32 [N,C,H,W]; do not write to the arrays."""
    return _table()


@functools.lru_cache(maxsize=None)
def reference(name):
    """loss_and_grad of a case of the table, computed once."""
    p, g, norm = cases()[name]
    return loss_and_grad(p, g, norm)


def sign_margin(name):
    """The smallest |Re F| or |Im F| over the bins that are not structural zeros, relative to max |F|: the guard that
    keeps the discontinuous sign from hiding a failure (a bin this close to zero could flip between two correct
    implementations)."""
    p, g, norm = cases()[name]
    d = p.astype(np.float64) - g.astype(np.float64)
    fre, fim = spectrum(d, norm)
    top = max(np.abs(fre).max(), np.abs(fim).max())
    free = ~np.broadcast_to(structural_zero(*d.shape[-2:]), fim.shape)
    assert (fim[~free] == 0).all()
    low = min(np.abs(fre).min(), np.abs(fim[free]).min() if free.any() else np.inf)
    return low, top
