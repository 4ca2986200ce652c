"""ops.layer_norm and ops.gelu on the GPU against fp64 torch: every output of both directions, repeated calls, the 4-D NHWC
form, and GELU's tail and misaligned paths.

Bars: values within 1e-4, gradients within 1e-3 of fp64, relative to the reference tensor's maximum."""
import pytest
import torch
import torch.nn.functional as F

import swinir_ref as R

pytestmark = pytest.mark.gpu

TOL_FWD, TOL_GRAD = 1e-4, 1e-3

# one row and one column; rows that do not fill a block, C below a wave; C = 60 and 180 (the two nets), the latter with more
# rows than one range of the parameter-gradient pass holds and more ranges than one block; C = a wave exactly; C above 256
LN_SHAPES = [(1, 1), (37, 8), (5, 60), (4100, 180), (3, 64), (2, 257)]


def _ops():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg.ops


def _ln_inputs(shape, seed):
    c = shape[-1]
    return (R.rand(shape, seed, 2.0) + 0.3, R.rand((c,), seed + 1) + 1.0, R.rand((c,), seed + 2), R.rand(shape, seed + 3))


def _ln_ref(x, gamma, beta, g, eps=1e-5):
    x64, g64, b64 = (t.double().requires_grad_() for t in (x, gamma, beta))
    # the definition written out (F.layer_norm's own rounding leaves 1e-17 where C = 1 makes x - mean an exact zero)
    mu = x64.mean(-1, keepdim=True)
    y = (x64 - mu) / ((x64 - mu).pow(2).mean(-1, keepdim=True) + eps).sqrt() * g64 + b64
    assert R.worst(y, F.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps)) <= 1e-12
    y.backward(g.double())
    mean = x.double().mean(-1)
    rstd = (x.double().var(-1, unbiased=False) + eps).rsqrt()
    return y.detach(), mean.flatten(), rstd.flatten(), x64.grad, g64.grad, b64.grad


def _ln_run(gpu, x, gamma, beta, g):
    ops = _ops()
    xd, gd, bd = (t.to(gpu).requires_grad_() for t in (x, gamma, beta))
    y = ops.layer_norm(xd, gd, bd)
    y.backward(g.to(gpu))
    y2, mean, rstd = ops.layer_norm_stats(xd.detach(), gd.detach(), bd.detach())
    assert torch.equal(y2, y.detach())
    return y.detach(), mean, rstd, xd.grad, gd.grad, bd.grad


@pytest.mark.parametrize("shape", LN_SHAPES + [(2, 5, 7, 12)], ids=str)
def test_layer_norm_matches_fp64(gpu, shape):
    args = _ln_inputs(shape, 11)
    got, want = _ln_run(gpu, *args), _ln_ref(*args)
    names = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")
    errs = [R.worst(a, b) for a, b in zip(got, want)]
    print("layer_norm %-16s %s" % (shape, "  ".join("%s %.3e" % (n, e) for n, e in zip(names, errs))))
    for n, e in zip(names, errs):
        assert e <= (TOL_FWD if n in ("y", "mean", "rstd") else TOL_GRAD), (n, e)


@pytest.mark.parametrize("shape", [(37, 8), (4100, 180)], ids=str)
def test_layer_norm_two_calls_are_bit_equal(gpu, shape):
    args = _ln_inputs(shape, 12)
    for a, b in zip(_ln_run(gpu, *args), _ln_run(gpu, *args)):
        assert torch.equal(a, b)


def test_layer_norm_refuses_a_wrong_affine(gpu):
    with pytest.raises(ValueError, match="gamma"):
        _ops().layer_norm(torch.zeros(3, 8, device=gpu), torch.zeros(7, device=gpu), torch.zeros(8, device=gpu))


def _gelu_ref(x, g):
    x64 = x.double().requires_grad_()
    y = F.gelu(x64)
    y.backward(g.double())
    return y.detach(), x64.grad


# one element, a tail alone, vectors and a tail, more than one pass of the grid's first blocks and a tail
@pytest.mark.parametrize("n", [1, 5, 1027, 65536 + 3])
def test_gelu_matches_fp64(gpu, n):
    x, g = R.rand((n,), 21, 4.0), R.rand((n,), 22)
    xd = x.to(gpu).requires_grad_()
    y = _ops().gelu(xd)
    y.backward(g.to(gpu))
    want = _gelu_ref(x, g)
    errs = R.worst(y, want[0]), R.worst(xd.grad, want[1])
    print("gelu n = %-6d y %.3e  dx %.3e" % ((n,) + errs))
    assert errs[0] <= TOL_FWD and errs[1] <= TOL_GRAD


def test_gelu_on_a_view_one_element_in(gpu):
    """A view that starts 4 bytes into its storage takes the 4-byte kernels; nothing before or after it is touched."""
    n = 1027
    base, g = R.rand((n + 2,), 23, 4.0).to(gpu), R.rand((n,), 24)
    keep = base.clone()
    view = base[1:n + 1]
    assert view.data_ptr() % 16 == 4
    xd = view.detach().requires_grad_()
    assert xd.data_ptr() == view.data_ptr()
    y = _ops().gelu(xd)
    y.backward(g.to(gpu))
    want = _gelu_ref(keep[1:n + 1].cpu(), g)
    assert R.worst(y, want[0]) <= TOL_FWD and R.worst(xd.grad, want[1]) <= TOL_GRAD
    assert torch.equal(base, keep)


def test_gelu_saturates_cleanly(gpu):
    x = torch.tensor([-1e4, -30.0, -0.0, 0.0, 30.0, 1e4], device=gpu).requires_grad_()
    y = _ops().gelu(x)
    y.backward(torch.ones_like(y))
    assert torch.equal(y.detach().cpu(), torch.tensor([-0.0, -0.0, -0.0, 0.0, 30.0, 1e4]))
    assert torch.equal(x.grad.cpu(), torch.tensor([0.0, 0.0, 0.5, 0.5, 1.0, 1.0]))
