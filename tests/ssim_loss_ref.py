"""What tests/test_ssim_loss_cpu.py and tests/test_ssim_loss_gpu.py share: the SSIM training loss, 1 - mean(SSIM) of an
UNCLAMPED prediction against its target (float domain, L = 1; window, constants and valid positions of ssim_ref), in fp64
torch on the CPU with the gradient from autograd, and the case table.  Nothing here uses the package under test."""
import functools

import numpy as np
import torch

import ssim_ref as R


def _valid_filter(a):
    """11 x 11 separable Gaussian at the valid positions of [..., H, W] (plain slicing, fp64, differentiable)."""
    g = torch.from_numpy(R.window())
    mw, mh = a.shape[-1] - 10, a.shape[-2] - 10
    hx = sum(g[k] * a[..., :, k:k + mw] for k in range(11))
    return sum(g[k] * hx[..., k:k + mh, :] for k in range(11))


def ssim_loss(x, y):
    """1 - mean SSIM of fp64 tensors [N,C,H,W] (x unclamped): every plane and position weighs the same."""
    mx, my = _valid_filter(x), _valid_filter(y)
    vx, vy, cov = _valid_filter(x * x) - mx * mx, _valid_filter(y * y) - my * my, _valid_filter(x * y) - mx * my
    s = ((2 * mx * my + R.C1) * (2 * cov + R.C2)) / ((mx * mx + my * my + R.C1) * (vx + vy + R.C2))
    return 1 - s.mean()


def loss_and_grad(pred, gt):
    """(loss, d loss / d pred) of fp32 [N,C,H,W] arrays in fp64: (float, fp64 array)."""
    x = torch.from_numpy(np.asarray(pred, np.float64)).requires_grad_(True)
    y = torch.from_numpy(np.asarray(gt, np.float64))
    loss = ssim_loss(x, y)
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


def mix_loss(pixel, a):
    """The reference mix of Zhao et al.: (1 - a) * pixel(pred, t) + a * (1 - SSIM(pred, t)), for torch tensors of any
    float dtype (the window follows the prediction's)."""
    def loss(pred, t):
        return (1 - a) * pixel(pred, t) + a * ssim_loss(pred.double(), t.double()).to(pred.dtype)
    return loss


@functools.lru_cache(maxsize=None)
def _table():
    out = {}
    for name, (p, g) in R.cases().items():
        if name == "batch_rgb":
            p = np.where(np.isnan(p), np.float32(0), p)   # the NaN leaves; the predictions outside [0, 1] stay
        out[name] = (p, g)
    return out


def cases():
    """The table of ssim_ref.cases() without its NaN (name -> (pred, gt), fp32 [N,C,H,W]); do not write to the arrays."""
    return _table()


@functools.lru_cache(maxsize=None)
def reference(name):
    """loss_and_grad of a case of the table, computed once."""
    return loss_and_grad(*cases()[name])


def out_of_range(a):
    return (a < 0) | (a > 1)
