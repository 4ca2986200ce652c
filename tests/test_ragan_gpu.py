"""The relativistic average GAN loss on the GPU (ops.ragan_loss over csrc/ragan.hip) against fp64 autograd over the case
table of tests/esrgan_ref.py: the loss and both gradient rows, [B] and [B, 1] logits, a detached row, the seed contract of
the other losses, two calls with the same bits, and a replayed graph against the eager call.

Bars: the project's standing contracts -- the loss within 1e-4, gradients within 1e-3 of max |fp64 reference| -- plus
the smallest positive fp32 number, 2^-149: a pair of logits 120 apart has a discriminator loss of e^-120 ~ 8e-53, which
no fp32 store can hold (the fp64 host twin is held to it in tests/test_ragan_cpu.py)."""
import pytest
import torch

import esrgan_ref as E
import rdn_ref as R

pytestmark = pytest.mark.gpu

TOL_FWD, TOL_GRAD = 1e-4, 1e-3
FP32_TINY = 2.0 ** -149


def _within(got, want, tol):
    """(max |got - want| / max |want| for the log, whether the bar holds)."""
    want = want.double().cpu()
    diff = float((got.double().cpu() - want).abs().max())
    scale = float(want.abs().max())
    return diff / max(scale, 1e-300), diff <= tol * scale + FP32_TINY


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _run(ops, real, fake, for_generator, gpu, column=False, detach_real=False):
    shape = (-1, 1) if column else (-1,)
    r = real.to(gpu).reshape(shape).requires_grad_(not detach_real)
    f = fake.to(gpu).reshape(shape).requires_grad_(True)
    loss = ops.ragan_loss(r, f, for_generator)
    ops.backward(loss)
    return loss.detach(), r.grad, f.grad


@pytest.mark.parametrize("for_generator", [False, True])
@pytest.mark.parametrize("name", sorted(E.RAGAN_CASES))
def test_matches_autograd(gpu, name, for_generator):
    ops = _pkg().ops
    real, fake = E.RAGAN_CASES[name]
    want, wr, wf = E.ragan_grads(real, fake, for_generator)
    loss, dr, df = _run(ops, real, fake, for_generator, gpu)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and dr.shape == real.shape and df.shape == fake.shape
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dr).all()) and bool(torch.isfinite(df).all())
    (e0, ok0), (e1, ok1), (e2, ok2) = _within(loss, want, TOL_FWD), _within(dr, wr, TOL_GRAD), _within(df, wf, TOL_GRAD)
    print("ragan %s %s: loss %.3e, d_real %.3e, d_fake %.3e of max |ref|" % (name, "G" if for_generator else "D", e0, e1, e2))
    assert ok0 and ok1 and ok2
    # two calls give the same bits; [B, 1] logits are the same numbers
    loss2, dr2, df2 = _run(ops, real, fake, for_generator, gpu, column=True)
    assert dr2.shape == (real.numel(), 1) and torch.equal(loss2, loss)
    assert torch.equal(dr2.reshape(-1), dr) and torch.equal(df2.reshape(-1), df)
    # a detached real row (the generator's step): no gradient for it, the same loss and fake row
    loss3, none, df3 = _run(ops, real, fake, for_generator, gpu, detach_real=True)
    assert none is None and torch.equal(loss3, loss) and torch.equal(df3, df)


def test_the_host_twin_agrees(gpu):
    import ctypes
    pkg = _pkg()
    lib = pkg._lib.load()
    real, fake = E.RAGAN_CASES["B257"]
    for mode in (False, True):
        loss, dr, df = _run(pkg.ops, real, fake, mode, gpu)
        hl = ctypes.c_double()
        hr, hf = torch.empty(257, dtype=torch.float64), torch.empty(257, dtype=torch.float64)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        assert lib.srk_ragan_loss_host(p(real), p(fake), 257, int(mode), 1.0, ctypes.byref(hl), p(hr), p(hf)) == 0
        # the kernel computes in double as the twin does: they differ by the order of the sums, then one fp32 rounding
        assert abs(float(loss) - hl.value) <= 1e-6 * abs(hl.value)
        assert R.worst(dr, hr) <= 1e-6 and R.worst(df, hf) <= 1e-6


@pytest.mark.parametrize("for_generator", [False, True])
def test_weighted_term_and_loss_sum(gpu, for_generator):
    """The contract of the other losses: as a weighted term of a loss_sum the gradient arrives weighed, from the loss
    kernel itself, and a general upstream gradient scales the stored rows."""
    ops = _pkg().ops
    real, fake = E.RAGAN_CASES["B16"]
    _, wr, wf = E.ragan_grads(real, fake, for_generator)
    r, f = real.to(gpu).requires_grad_(True), fake.to(gpu).requires_grad_(True)
    other = ops.l1_loss(f.reshape(-1, 1), torch.zeros(16, 1, device=gpu))
    term = ops.weighted_term(lambda pred, target: ops.ragan_loss(target, pred, for_generator), 5e-3, f, r)
    total = ops.loss_sum(other, term, 1.0, 5e-3)
    ops.backward(total)
    l1g = torch.sign(fake.double()) / 16
    assert R.worst(r.grad, 5e-3 * wr) <= TOL_GRAD and R.worst(f.grad, 5e-3 * wf + l1g) <= TOL_GRAD
    r2, f2 = real.to(gpu).requires_grad_(True), fake.to(gpu).requires_grad_(True)
    (ops.ragan_loss(r2, f2, for_generator) * 3.0).backward()
    assert R.worst(r2.grad, 3 * wr) <= TOL_GRAD and R.worst(f2.grad, 3 * wf) <= TOL_GRAD


@pytest.mark.parametrize("for_generator", [False, True])
def test_replayed_graph_equals_eager(gpu, for_generator):
    pkg = _pkg()
    ops = pkg.ops
    real, fake = E.RAGAN_CASES["B16_extreme"]
    r, f = real.to(gpu), fake.to(gpu)

    def fn(r_in, f_in):
        a, b = r_in.detach().requires_grad_(True), f_in.detach().requires_grad_(True)
        loss = ops.ragan_loss(a, b, for_generator)
        ops.backward(loss)
        return loss, a.grad, b.grad

    eager = [t.clone() for t in fn(r, f)]
    graph = pkg.trainers.capture_step(fn, [r, f], warmup=0)
    other = E.RAGAN_CASES["B16"]
    graph(other[0].to(gpu), other[1].to(gpu))            # another batch in between
    got = [t.clone() for t in graph(r, f)]
    graph.close()
    for a, b in zip(eager, got):
        assert torch.equal(a, b)


def test_shapes_are_checked(gpu):
    ops = _pkg().ops
    with pytest.raises(ValueError, match="real_logits"):
        ops.ragan_loss(torch.zeros(4, 2, device=gpu), torch.zeros(4, device=gpu), False)
    with pytest.raises(ValueError, match="4 real logits vs 3 fake"):
        ops.ragan_loss(torch.zeros(4, device=gpu), torch.zeros(3, device=gpu), False)
    with pytest.raises(ValueError, match="fake_logits"):
        ops.ragan_loss(torch.zeros(4, device=gpu), torch.zeros(4, 1, 1, device=gpu), True)
    with pytest.raises(ValueError, match="B >= 1"):
        ops.ragan_loss(torch.zeros(0, device=gpu), torch.zeros(0, device=gpu), True)
