"""tests/streaming_ref.py against torch in float64, and the bars of test_streaming_gpu.py against float32: the same
formulas evaluated by torch in fp32 on the CPU, on the inputs the GPU file uses, stay within HALF of each bar -- so a
bar is reachable by fp32 arithmetic with head-room, and (the fractions are far from zero) not vacuous either.  The
planted-mass inputs of the reductions are checked here for what they promise."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import streaming_ref as R
from streaming_ref import BAR, f32

HALF = 0.5


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a)).to(dtype)      # (a copy: optimizers update in place)


def _torch_act(x, kind, slope, w):
    if kind == "relu":
        return F.relu(x)
    if kind == "lrelu":
        return F.leaky_relu(x, slope)
    if kind in ("prelu", "prelu_c"):
        return F.prelu(x.movedim(-1, 1), w).movedim(1, -1)
    return torch.tanh(x) if kind == "tanh" else torch.sigmoid(x)


# ---- the references are the formulas torch implements -----------------------------------------------------------------
@pytest.mark.parametrize("kind", R.ACTS)
def test_ref_activation_is_torch_fp64(kind):
    C = 6
    x, dy = R.gen_act(40 * C)
    x, dy = x.reshape(5, 8, C), dy.reshape(5, 8, C)
    w = {"prelu": R.gen_prelu_w(1), "prelu_c": R.gen_prelu_w(C)}.get(kind)
    slope = f32(0.2)
    xt = _t(x).requires_grad_(True)
    wt = _t(w).requires_grad_(True) if w is not None else None
    yt = _torch_act(xt, kind, slope, wt)
    yt.backward(_t(dy))
    y = R.act_fwd(x, kind, slope, w)
    assert np.abs(y - yt.detach().numpy()).max() <= 1e-15
    dx, dw = R.act_bwd(dy, x if w is not None else y, kind, slope, w)
    assert np.abs(dx - xt.grad.numpy()).max() <= 1e-14
    if w is not None:
        assert np.abs(dw - wt.grad.numpy()).max() <= 1e-13
    # torch's conventions at +-0: relu' = 0, the slope side for prelu / lrelu
    z = np.array([0.0, -0.0], np.float32)
    w1 = w[:1] if w is not None else None
    dz, _ = R.act_bwd(np.ones(2), z if w is not None else R.act_fwd(z, kind, slope), kind, slope, w1)
    zt = _t(z).requires_grad_(True)
    _torch_act(zt.reshape(1, 2, 1), kind, slope, wt[:1] if wt is not None else None).sum().backward()
    assert np.array_equal(dz, zt.grad.numpy())


@pytest.mark.parametrize("kind", R.LOSSES)
def test_ref_loss_is_torch_fp64(kind):
    p, t = R.gen_loss(kind, 1025, R.positions(1025, 1))
    if kind == "bce":
        p[:4], t[:4] = (0.0, 0.0, 1.0, 1.0), (0.0, 1.0, 0.0, 1.0)    # the clamps
    eps = f32(1e-6)
    pt = _t(p).requires_grad_(True)
    fn = {"mse": F.mse_loss, "l1": F.l1_loss, "bce": F.binary_cross_entropy,
          "charbonnier": lambda a, b: torch.sqrt((a - b) ** 2 + eps).mean()}[kind]
    lt = fn(pt, _t(t))
    lt.backward()
    val, g = R.loss(kind, p, t, eps)
    assert abs(val - lt.item()) <= 1e-13 * abs(lt.item())
    assert R.frac_of_bar(g, pt.grad.numpy(), rtol=1e-12, atol=0.0) <= 1.0


@pytest.mark.parametrize("variant", sorted(R.SGD_VARIANTS))
@pytest.mark.parametrize("gs", [1.0, 0.25])
def test_ref_sgd_is_torch_fp64(variant, gs):
    p0, grads = R.gen_opt(1023)
    hp = R.SGD_VARIANTS[variant]
    pt = _t(p0).requires_grad_(True)
    opt = torch.optim.SGD([pt], lr=R.SGD_LR, momentum=hp["mom"], weight_decay=hp["wd"], nesterov=hp["nesterov"])
    for g in grads:
        pt.grad = _t(g) * gs
        opt.step()
    p, buf = R.run_sgd(p0, grads, variant, gs)
    assert np.abs(p - pt.detach().numpy()).max() <= 1e-14
    if hp["mom"]:
        assert np.abs(buf - opt.state[pt]["momentum_buffer"].numpy()).max() <= 1e-13
    # first = True ignores the buffer, first = False on a zero buffer gives the same step (optim.SGD's zero-filled start)
    a = R.sgd_step(p0, grads[0], np.full(1023, np.nan), R.SGD_LR, first=True, **hp)
    b = R.sgd_step(p0, grads[0], np.zeros(1023), R.SGD_LR, first=False, **hp)
    assert np.array_equal(a[0], b[0]) and np.isfinite(a[0]).all()


@pytest.mark.parametrize("wd", [0.0, f32(1e-4)])
def test_ref_adam_is_torch_fp64(wd):
    p0, grads = R.gen_opt(1023)
    pt = _t(p0).requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=R.ADAM["lr"], betas=(R.ADAM["b1"], R.ADAM["b2"]), eps=R.ADAM["eps"], weight_decay=wd)
    for g in grads:
        pt.grad = _t(g)
        opt.step()
    p, m, v, t = R.run_adam(p0, grads, wd)
    st = opt.state[pt]
    assert t == 3 == int(st["step"])
    assert R.frac_of_bar(p, pt.detach().numpy(), rtol=1e-13) <= 1.0
    assert R.frac_of_bar(m, st["exp_avg"].numpy(), rtol=1e-13) <= 1.0
    assert R.frac_of_bar(v, st["exp_avg_sq"].numpy(), rtol=1e-13) <= 1.0
    moved = np.abs(p - p0) / np.abs(p0)
    live = np.abs(grads[0]) > 1e-6
    assert 0.03 < np.median(moved[live]) < 0.3 and moved.max() <= 0.31     # a step error of 1e-5 is not under p's rounding


def test_ref_clip_and_rest_are_torch():
    g = R.gen_mass(4099, R.positions(4099, 3))
    for max_norm in (0.5, 10.0):
        gt = _t(g).requires_grad_(True)
        gt.grad = _t(g).clone()
        tn = torch.nn.utils.clip_grad_norm_([gt], max_norm)
        norm, scale = R.clip(g, max_norm)
        assert abs(norm - float(tn)) <= 1e-13 * norm
        assert np.abs(gt.grad.numpy() - g.astype(np.float64) * scale).max() <= 1e-15
        assert (scale < 1.0) == (max_norm < norm)
    x = R._rs(1).standard_normal((2, 3, 5, 7)).astype(np.float32)
    for r in (2, 3):
        assert np.array_equal(R.upsample_fwd(x, r), F.interpolate(_t(x, torch.float32), scale_factor=r, mode="nearest").numpy())
        gy = _t(R._rs(2).standard_normal((2, 3, 5 * r, 7 * r)))
        xt = _t(x).requires_grad_(True)
        F.interpolate(xt, scale_factor=r, mode="nearest").backward(gy)
        assert np.abs(R.upsample_bwd(gy.numpy(), r) - xt.grad.numpy()).max() <= 1e-14
    assert np.array_equal(R.maxpool2(x), F.max_pool2d(_t(x, torch.float32), 2, 2).numpy())
    sub, div = (0.4, 0.5, 0.6), (0.2, 0.25, 0.3)
    assert np.array_equal(R.channel_affine(x, [f32(s) for s in sub], [f32(d) for d in div], dt=np.float32),
                          _t(x, torch.float32).sub(torch.tensor(sub).view(1, 3, 1, 1)).div(torch.tensor(div).view(1, 3, 1, 1)).numpy())
    pr, gt_ = R._rs(3).uniform(-0.2, 1.2, 300).astype(np.float32), R._rs(4).uniform(size=300).astype(np.float32)
    ps, mse = R.psnr(pr, gt_)
    d = torch.from_numpy(pr).clamp(0, 1) - torch.from_numpy(gt_)
    assert abs(mse - float(d.double().pow(2).mean())) <= 1e-15 and abs(ps - 10 * np.log10(1 / mse)) <= 1e-12
    assert R.psnr(gt_, gt_) == (100.0, 0.0)
    assert R.absmax([-3.0, 2.0, -0.0]) == 3.0


# ---- fp32 on the CPU stays within half of every bar -------------------------------------------------------------------
ACT_N = (4099, R.CAP_EW + 3)


@pytest.mark.parametrize("kind", R.ACTS)
def test_bar_activation(kind):
    for n in ACT_N if kind in ("lrelu", "tanh", "sigmoid") else ACT_N[:1]:
        C = 1 if n % 8 else 8
        if kind == "prelu_c":
            n, C = 4096 + 8, 8
        x, dy = R.gen_act(n)
        x, dy = x.reshape(-1, C), dy.reshape(-1, C)
        w = {"prelu": R.gen_prelu_w(1), "prelu_c": R.gen_prelu_w(C)}.get(kind)
        if w is not None:
            dy = np.abs(dy)      # (as the GPU file: the slope gradient is a sum without cancellation)
        slope = f32(0.2)
        xt = _t(x, torch.float32).requires_grad_(True)
        wt = _t(w, torch.float32).requires_grad_(True) if w is not None else None
        yt = _torch_act(xt, kind, slope, wt)          # torch fp32: stands in for the device's y
        yt.backward(_t(dy, torch.float32))
        y32 = yt.detach().numpy()
        assert R.frac_of_bar(y32, R.act_fwd(x, kind, slope, w)) <= HALF
        # backward from the tensor the kernel reads: the fp32 output
        saved = x if w is not None else y32
        dx, dw = R.act_bwd(dy, saved, kind, slope, w)
        dx32, dw32 = R.act_bwd(dy, saved, kind, slope, w, dt=np.float32)
        assert R.frac_of_bar(dx32, dx) <= HALF
        if kind in ("relu", "lrelu", "prelu", "prelu_c"):          # (torch's own backward reads x: same masks)
            assert R.frac_of_bar(xt.grad.numpy(), dx) <= HALF
        if w is not None:
            assert R.frac_of_bar(wt.grad.numpy(), dw, rtol=R.BAR_DPRELU) <= HALF


LOSS_N = (4099, R.CAP_LOSS4 + 4, R.CAP_RED + 3)


@pytest.mark.parametrize("kind", R.LOSSES)
def test_bar_loss_and_planted_mass(kind):
    eps = f32(1e-6)
    for n in LOSS_N:
        where = R.positions(n, R.grid_loss(n, n % 4 == 0), 4 if n % 4 == 0 else 1)
        p, t = R.gen_loss(kind, n, where)
        val, g = R.loss(kind, p, t, eps)
        pt = _t(p, torch.float32).requires_grad_(True)
        fn = {"mse": F.mse_loss, "l1": F.l1_loss, "bce": F.binary_cross_entropy,
              "charbonnier": lambda a, b: torch.sqrt((a - b) ** 2 + eps).mean()}[kind]
        lt = fn(pt, _t(t, torch.float32))
        lt.backward()
        assert abs(lt.item() - val) <= HALF * BAR * abs(val), (kind, n, lt.item(), val)
        regular = np.ones(n, bool)
        regular[where] = False
        atol = BAR * float(np.sqrt(np.mean(g[regular] ** 2)))
        assert R.frac_of_bar(pt.grad.numpy(), g, atol=atol) <= HALF
        # planted mass: leaving out (or repeating) any ONE of the structural elements moves the mean by > 100 bars
        for i in where:
            one, _ = R.loss(kind, p[i:i + 1], t[i:i + 1], eps)
            assert one / n > 100 * BAR * val, (kind, n, i, one / n / val)


@pytest.mark.parametrize("n", [4099, R.CAP_RED + 3, R.CAP_RED + 4])
def test_bar_norm_and_planted_mass(n):
    where = R.positions(n, R.grid_red(n))
    g = R.gen_mass(n, where)
    norm, _ = R.clip(g, 1.0)
    # fp32 squares, wide accumulation (the kernels sum block partials in double), the norm rounded to fp32
    n32 = float(np.float32(np.sqrt(np.sum(g * g, dtype=np.float64))))
    assert abs(n32 - norm) <= HALF * BAR * norm
    for i in where:
        assert abs(np.sqrt(norm ** 2 - float(g[i]) ** 2) - norm) > 100 * BAR * norm
    # PSNR's mse over the same vector as the difference
    gt = R._rs(7).uniform(0.25, 0.75, n).astype(np.float32)
    pred = gt + g * np.float32(0.25)
    _, mse = R.psnr(pred, gt)
    for i in where:
        d = np.float32(pred[i]) - gt[i]
        assert float(d) ** 2 / n > 100 * BAR * mse


@pytest.mark.parametrize("variant", sorted(R.SGD_VARIANTS))
def test_bar_sgd(variant):
    hp = R.SGD_VARIANTS[variant]
    for n, gs in ((4099, 1.0), (R.CAP_RED + 3, 0.25)):
        p0, grads = R.gen_opt(n)
        pt = _t(p0, torch.float32).requires_grad_(True)
        opt = torch.optim.SGD([pt], lr=R.SGD_LR, momentum=hp["mom"], weight_decay=hp["wd"], nesterov=hp["nesterov"])
        for g in grads:
            pt.grad = _t(g, torch.float32) * gs
            opt.step()
        p, buf = R.run_sgd(p0, grads, variant, gs)
        assert R.frac_of_bar(pt.detach().numpy(), p) <= HALF
        if hp["mom"]:
            assert R.frac_of_bar(opt.state[pt]["momentum_buffer"].numpy(), buf) <= HALF


@pytest.mark.parametrize("wd", [0.0, f32(1e-4)])
def test_bar_adam(wd):
    for n in (17, 4099, R.CAP_ADAM4 + 4):
        p0, grads = R.gen_opt(n)
        pt = _t(p0, torch.float32).requires_grad_(True)
        opt = torch.optim.Adam([pt], lr=R.ADAM["lr"], betas=(R.ADAM["b1"], R.ADAM["b2"]), eps=R.ADAM["eps"], weight_decay=wd)
        for g in grads:
            pt.grad = _t(g, torch.float32)
            opt.step()
        p, m, v, _ = R.run_adam(p0, grads, wd)
        st = opt.state[pt]
        assert R.frac_of_bar(pt.detach().numpy(), p) <= HALF
        assert R.frac_of_bar(st["exp_avg"].numpy(), m) <= HALF
        assert R.frac_of_bar(st["exp_avg_sq"].numpy(), v) <= HALF


def test_bar_axpby_affine_upsample_bwd():
    a, b = R.gen_act(R.CAP_EW + 3)
    assert R.frac_of_bar(a + b, a.astype(np.float64) + b) <= HALF
    al, be = f32(0.3), f32(-1.7)
    assert R.frac_of_bar(np.float32(al) * a + np.float32(be) * b, al * a.astype(np.float64) + be * b) <= HALF
    x = R._rs(9).standard_normal((2, 3, 31, 33)).astype(np.float32)
    sub, div = [f32(v) for v in (0.4, 0.5, 0.6)], [f32(v) for v in (0.2, 0.25, 0.3)]
    assert R.frac_of_bar(R.channel_affine(x, sub, div, dt=np.float32), R.channel_affine(x, sub, div)) <= HALF
    gy = R._rs(10).standard_normal((2, 3, 31 * 4, 33 * 4)).astype(np.float32)
    xt = _t(x, torch.float32).requires_grad_(True)
    F.interpolate(xt, scale_factor=4, mode="nearest").backward(_t(gy, torch.float32))
    assert R.frac_of_bar(xt.grad.numpy(), R.upsample_bwd(gy, 4)) <= HALF
