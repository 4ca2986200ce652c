"""The perceptual (VGG feature) loss on the MI355X: the max-pool gradient kernel bit for bit against ATen's CPU autograd,
the VGG head with a gradient, ops.perceptual_loss and the SRGAN step that trains on it -- against the float64 CPU
yardstick of tests/perceptual_ref.py (bars: see there), eager, captured, pruned, data-parallel and from the command line."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import perceptual_ref as P
from conftest import rel_err
from oracle import fill, ref_modules as R

pytestmark = pytest.mark.gpu
ROOT = P.ROOT
CL = torch.channels_last


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _fmt(t, channels_last):
    return t.contiguous(memory_format=CL) if channels_last else t.contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# pool backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.POOL_KINDS)
@pytest.mark.parametrize("shape", P.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_backward_bit_exact(gpu, shape, kind):
    """ops.max_pool2x2_train against max_pool2d's autograd on the CPU, torch.equal, x and dy each NCHW-dense and
    channels_last: odd H / W (trailing zeros), C in {1, 3, 5} (scalar path) and C % 4 == 0 (16-byte path), ties."""
    pkg = _pkg()
    n, c, h, w = shape
    x = P.pool_input(shape, kind)
    dy = fill.randn((n, c, h // 2, w // 2), 741)
    for x_cl in (False, True):
        for dy_cl in (False, True):
            xc, dyc = _fmt(x, x_cl), _fmt(dy, dy_cl)
            want = P.pool_grad_cpu(xc, dyc)
            xd = xc.to(gpu).requires_grad_(True)
            y = pkg.ops.max_pool2x2_train(xd)
            assert y.requires_grad and torch.equal(y.detach().cpu(), nn.functional.max_pool2d(x, 2, 2))
            y.backward(dyc.to(gpu))
            assert torch.equal(xd.grad.cpu(), want), (shape, kind, x_cl, dy_cl)


def _pool_bwd_raw(pkg, x_nhwc, dy_nhwc, dx_nhwc, n, h, w, c, relu_input):
    lib = pkg._lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.srk_maxpool2x2_backward(p(x_nhwc), p(dy_nhwc), p(dx_nhwc), n, h, w, c, relu_input, pkg._lib.stream_ptr()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", P.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_backward_writes_every_element(gpu, shape):
    """srk_maxpool2x2_backward on a dx pre-filled with NaN: every element is written, the zeros of an odd trailing
    row / column included; the same through pointers that are not 16-byte aligned (scalar path at C % 4 == 0)."""
    pkg = _pkg()
    n, c, h, w = shape
    x = P.pool_input(shape, "continuous")
    dy = fill.randn((n, c, h // 2, w // 2), 742)
    want = P.pool_grad_cpu(x, dy)
    for off in (0, 1):     # element offset of all three buffers from their (256-byte aligned) allocations
        bufs = []
        for t in (x, dy):
            flat = torch.empty(t.numel() + 1, device=gpu)
            v = flat[off:off + t.numel()].view(t.shape[0], t.shape[2], t.shape[3], t.shape[1])
            v.copy_(t.permute(0, 2, 3, 1))
            bufs.append(v)
        flat = torch.full((x.numel() + 2,), float("nan"), device=gpu)
        dx = flat[off:off + x.numel()].view(n, h, w, c)
        assert dx.data_ptr() % 16 == 4 * off
        _pool_bwd_raw(pkg, bufs[0], bufs[1], dx, n, h, w, c, 0)
        assert not torch.isnan(dx).any(), (shape, off)
        assert torch.equal(dx.permute(0, 3, 1, 2).cpu(), want), (shape, off)
        assert torch.isnan(flat[off + x.numel():]).all() and (off == 0 or torch.isnan(flat[0]))   # nothing outside dx


@pytest.mark.parametrize("shape", P.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_backward_relu_input(gpu, shape):
    """relu_input = 1: with x = relu(z), z continuous, dx is torch's gradient of max_pool2d(relu(z)) with respect to z --
    the pool's gradient already multiplied by the ReLU's mask -- bit for bit."""
    pkg = _pkg()
    n, c, h, w = shape
    z = fill.randn(shape, 743)
    z[:, :, :2, :2] = -z[:, :, :2, :2].abs()      # a window without a positive value: routes nothing
    dy = fill.randn((n, c, h // 2, w // 2), 744)
    zr = z.clone().requires_grad_(True)
    nn.functional.max_pool2d(torch.relu(zr), 2, 2).backward(dy)
    xd = torch.relu(z).permute(0, 2, 3, 1).contiguous().to(gpu)
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(gpu)
    dx = torch.full((n, h, w, c), float("nan"), device=gpu)
    _pool_bwd_raw(pkg, xd, dyd, dx, n, h, w, c, 1)
    assert torch.equal(dx.permute(0, 3, 1, 2).cpu(), zr.grad), shape
    assert not dx[:, :2, :2, :].any()


def test_pool_mark_reaches_the_conv_below(gpu):
    """conv + ReLU -> pool inside premasked_gradients(): the pool launches with relu_input = 1, marks its dx, and the
    conv skips its mask read (masks_skipped rises by exactly one); the input gradient is the one of the standard
    protocol (same kernels, the 0 / 1 mask applied once instead of twice: compared at 1e-6 of its maximum).  Outside the
    context no mark is set."""
    pkg = _pkg()
    ops = pkg.ops
    conv = pkg.layers.Conv2d(8, 16, 3, 1, 1)
    fill.fill_module(conv, 11)
    conv.to(gpu)
    x = fill.randn((2, 8, 9, 7), 745).to(gpu)
    g = fill.randn((2, 16, 4, 3), 746).to(gpu)
    res = {}
    for premask in (False, True):
        xr = x.clone().requires_grad_(True)
        y = ops.max_pool2x2_train(ops.conv2d(xr, conv.weight, conv.bias, None, ops.ConvCfg(1, 1, False, 0, pkg._lib.ACT_RELU)))
        before = dict(ops.PREMASK_STATS)
        if premask:
            with ops.premasked_gradients():
                y.backward(g)
        else:
            y.backward(g)
        res[premask] = (xr.grad.clone(), ops.PREMASK_STATS["masks_skipped"] - before["masks_skipped"],
                        ops.PREMASK_STATS["masked_dx"] - before["masked_dx"])
    assert res[False][1:] == (0, 0) and res[True][1:] == (1, 1)
    err, scale = P.max_err(res[True][0], res[False][0])
    assert scale > 0 and err <= 1e-6 * scale


# ---------------------------------------------------------------------------------------------------------------------
# head with gradient
# ---------------------------------------------------------------------------------------------------------------------
_FE = {}


def _extractor(pkg, gpu, feature_layer=8, seed=77):
    key = (feature_layer, seed)
    if key not in _FE:
        _FE[key] = pkg.FeatureExtractor(feature_layer=feature_layer).load_vgg19(P.filled_head(feature_layer, seed)[2]).to(gpu)
    return _FE[key]


def _hold(what, got, ref, contract, err32):
    err, scale = P.max_err(got, ref)
    bound = P.bar(contract, err32, scale)
    print("%-34s max|ref| %.4e  err %.3e (%.2e rel)  torch fp32 CPU err %.3e  contract %.3e  bar %.3e"
          % (what, scale, err, err / max(scale, 1e-300), err32, contract * scale, bound))
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("feature_layer,shape", P.HEAD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_head_with_gradient(gpu, feature_layer, shape):
    """FeatureExtractor.extract(x, grad=True): features and d sum(features * g) / dx against float64; forward() still
    detached; no parameter gradient."""
    pkg = _pkg()
    fe = _extractor(pkg, gpu, feature_layer)
    case = P.head_case(feature_layer, shape)
    x = case["x"].to(gpu).requires_grad_(True)
    f = fe.extract(x, grad=True)
    assert f.requires_grad and tuple(f.shape) == tuple(case["f64"].shape)
    (f * case["g"].to(gpu)).sum().backward()
    tag = "layer %d %s " % (feature_layer, "x".join(map(str, shape)))
    _hold(tag + "features", f, case["f64"], P.OUT_CONTRACT, case["f_err32"])
    _hold(tag + "dx", x.grad, case["dx64"], P.GRAD_CONTRACT, case["dx_err32"])
    out = fe(x)
    assert not out.requires_grad
    _hold(tag + "forward()", out, case["f64"], P.OUT_CONTRACT, case["f_err32"])
    assert not fe.extract(x).requires_grad                      # grad=False is forward()
    assert all(p.grad is None and not p.requires_grad for p in fe.parameters())


def test_head_packs_are_cached(gpu):
    """Both filter packs of every head layer come from the layer's cache: a second differentiable walk (after an
    optimizer-step epoch bump) packs nothing; load_vgg19 drops them."""
    pkg = _pkg()
    fe = pkg.FeatureExtractor().load_vgg19(P.filled_head(8)[2]).to(gpu)
    convs = [m for m in fe.features if isinstance(m, nn.Conv2d)]
    x = P.head_case(8, (1, 3, 9, 7))["x"].to(gpu).requires_grad_(True)
    fe.extract(x, grad=True).sum().backward()
    packs = [(m._cache.val[0].data_ptr(), m._cache.bwd.data_ptr()) for m in convs]
    pkg.layers.bump_weight_epoch()
    calls = []
    orig_f, orig_b = pkg.ops.pack_weight_fwd, pkg.ops.pack_weight_bwd
    pkg.ops.pack_weight_fwd = lambda *a, **k: (calls.append("fwd"), orig_f(*a, **k))[1]
    pkg.ops.pack_weight_bwd = lambda *a, **k: (calls.append("bwd"), orig_b(*a, **k))[1]
    try:
        fe.extract(x, grad=True).sum().backward()
        assert calls == []
        assert packs == [(m._cache.val[0].data_ptr(), m._cache.bwd.data_ptr()) for m in convs]
        fe.load_vgg19(P.filled_head(8, 78)[2])
        assert all(m._cache.key is None for m in convs)
        fe.extract(x, grad=True).sum().backward()
        assert sorted(calls) == ["bwd"] * len(convs) + ["fwd"] * len(convs)
    finally:
        pkg.ops.pack_weight_fwd, pkg.ops.pack_weight_bwd = orig_f, orig_b


# ---------------------------------------------------------------------------------------------------------------------
# loss
# ---------------------------------------------------------------------------------------------------------------------
def _loss_and_grad(pkg, gpu, fe, case, premask=False, wrap=None):
    pred = case["pred"].to(gpu).requires_grad_(True)
    target = case["target"].to(gpu)
    loss = (wrap or (lambda p, t: pkg.ops.perceptual_loss(p, t, fe)))(pred, target)
    if premask:
        with pkg.ops.premasked_gradients():
            loss.backward()
    else:
        loss.backward()
    return loss.detach(), pred.grad


def _hold_loss(tag, loss, case):
    err = abs(float(loss) - case["l64"])
    bound = P.bar(P.OUT_CONTRACT, case["l_err32"], abs(case["l64"]))
    print("%-34s ref %.6e  err %.3e  torch fp32 CPU err %.3e  bar %.3e" % (tag, case["l64"], err, case["l_err32"], bound))
    assert err <= bound, (tag, err, bound)


@pytest.mark.parametrize("shape", P.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradient(gpu, shape):
    """ops.perceptual_loss and d loss / d pred against float64; the nn.Module twin is the same call; the same gradient
    taken inside premasked_gradients() meets the same bar and skips at least one mask read."""
    pkg = _pkg()
    fe = _extractor(pkg, gpu)
    case = P.loss_case(shape)
    tag = "loss %s " % "x".join(map(str, shape))
    loss, grad = _loss_and_grad(pkg, gpu, fe, case)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    _hold_loss(tag + "value", loss, case)
    _hold(tag + "d/dpred", grad, case["d64"], P.GRAD_CONTRACT, case["d_err32"])
    mod = pkg.utils.PerceptualLoss(fe)
    loss_m, grad_m = _loss_and_grad(pkg, gpu, fe, case, wrap=mod)
    assert torch.equal(loss_m, loss) and torch.equal(grad_m, grad)
    before = pkg.ops.PREMASK_STATS["masks_skipped"]
    loss_p, grad_p = _loss_and_grad(pkg, gpu, fe, case, premask=True)
    assert pkg.ops.PREMASK_STATS["masks_skipped"] >= before + 1
    assert torch.equal(loss_p, loss)
    _hold(tag + "d/dpred premasked", grad_p, case["d64"], P.GRAD_CONTRACT, case["d_err32"])


def test_loss_of_equal_operands_is_exactly_zero(gpu):
    """perceptual_loss(x, x): both operands run the same kernels, so the loss is 0.0 and the gradient holds no nonzero."""
    pkg = _pkg()
    fe = _extractor(pkg, gpu)
    for shape in P.LOSS_SHAPES:
        x = P.loss_case(shape)["pred"].to(gpu)
        pred = x.clone().requires_grad_(True)
        loss = pkg.ops.perceptual_loss(pred, x, fe)
        loss.backward()
        assert float(loss) == 0.0 and not pred.grad.any(), shape
        pred = x.contiguous(memory_format=CL).clone().requires_grad_(True)       # the layouts of the two may differ
        loss = pkg.ops.perceptual_loss(pred, x, fe, normalize=False)
        loss.backward()
        assert float(loss) == 0.0 and not pred.grad.any(), shape


def test_loss_target_gets_no_gradient_and_shapes_are_checked(gpu):
    pkg = _pkg()
    fe = _extractor(pkg, gpu)
    case = P.loss_case((1, 3, 9, 7))
    pred = case["pred"].to(gpu).requires_grad_(True)
    target = case["target"].to(gpu).requires_grad_(True)
    pkg.ops.perceptual_loss(pred, target, fe).backward()
    assert target.grad is None and pred.grad is not None and pred.grad.any()
    for bad in ((1, 1, 9, 7), (1, 4, 9, 7), (3, 9, 7)):
        with pytest.raises(ValueError):
            pkg.ops.perceptual_loss(torch.zeros(bad, device=gpu), torch.zeros(bad, device=gpu), fe)
    with pytest.raises(ValueError):
        pkg.ops.perceptual_loss(torch.zeros((1, 3, 8, 8), device=gpu), torch.zeros((1, 3, 8, 6), device=gpu), fe)


def test_loss_as_a_weighted_term(gpu):
    """Under ops.weighted_term(.., 6e-3, ..) + ops.loss_sum + the unit seed -- how the step uses it -- the gradient is
    6e-3 times the plain one (the weight is folded into the MSE kernel's gradient: rounding differs, the gradient bar
    holds) and the sum is other + 6e-3 * term."""
    pkg = _pkg()
    ops = pkg.ops
    fe = _extractor(pkg, gpu)
    case = P.loss_case((2, 3, 12, 10))
    _, plain = _loss_and_grad(pkg, gpu, fe, case)
    pred = case["pred"].to(gpu).requires_grad_(True)
    target = case["target"].to(gpu)
    term = ops.weighted_term(lambda p, t: ops.perceptual_loss(p, t, fe), 6e-3, pred, target)
    other = ops.mse_loss(case["pred"].to(gpu), target)
    total = ops.loss_sum(other, term, 1.0, 6e-3)
    ops.backward(total)
    assert abs(float(total) - (float(other) + 6e-3 * float(term))) <= 1e-6 * abs(float(total))
    _hold("weighted term d/dpred", pred.grad, 6e-3 * case["d64"], P.GRAD_CONTRACT, 6e-3 * case["d_err32"])
    err, scale = P.max_err(pred.grad, 6e-3 * plain.double())
    assert err <= P.GRAD_CONTRACT * scale


# ---------------------------------------------------------------------------------------------------------------------
# step
# ---------------------------------------------------------------------------------------------------------------------
def _batch(gpu):
    return fill.rand((2, 3, 8, 8), 670).to(gpu), fill.rand((2, 3, 32, 32), 671).to(gpu)


def _make_step(pkg, gpu, perceptual, **kw):
    G, D = pkg.SRGANGenerator(3, 16, 2), pkg.SRGANDiscriminator(3, 8, 32)
    fill.fill_module(G, 5, 0.7)
    fill.fill_module(D, 6, 1.0)
    G.to(gpu).train()
    D.to(gpu).train()
    g_flat, d_flat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
    g_opt = pkg.optim.make_optimizer("srgan_g", g_flat, 1e-3)
    d_opt = pkg.optim.make_optimizer("srgan_d", d_flat, 1e-2)
    fe = _extractor(pkg, gpu, 8, 78)
    step = pkg.trainers.srgan_step(G, D, g_opt, d_opt, feature_extractor=fe, perceptual=perceptual, **kw)
    return G, D, g_flat, d_flat, g_opt, d_opt, step


def _oracle_step_with_term():
    """srgan.py:249-310 in fp32 on the CPU (oracle.ref_modules nets, stock VGG head) with the term ATTACHED to recon."""
    head = P.filled_head(8, 78)[0]
    lr_img, hr_img = fill.rand((2, 3, 8, 8), 670), fill.rand((2, 3, 32, 32), 671)
    G = fill.fill_module(R.Generator(3, 16, 2), 5, 0.7).train()
    D = fill.fill_module(R.Discriminator(3, 8, 32), 6, 1.0).train()
    g_opt = R.make_optimizer("srgan_g", G.parameters(), 1e-3)
    d_opt = R.make_optimizer("srgan_d", D.parameters(), 1e-2)
    bce, mse = nn.BCELoss(), nn.MSELoss()
    real, fake = torch.ones(2, 1), torch.zeros(2, 1)
    d_opt.zero_grad()
    d_loss = bce(D(hr_img), real) + bce(D(G(lr_img)), fake)
    d_loss.backward()
    d_opt.step()
    g_opt.zero_grad()
    recon = G(lr_img)
    vgg = mse(head(P.vnorm(recon)), head(P.vnorm(hr_img)).detach())
    g_loss = mse(recon, hr_img) + 6e-3 * vgg + 1e-3 * bce(D(recon), real)
    g_loss.backward()
    g_opt.step()
    return float(d_loss), float(g_loss), float(vgg), G


def test_step_trains_on_the_term(gpu):
    """perceptual=True against perceptual=False with the same extractor: D's side is untouched bit for bit, G's update
    differs, the reported G loss is the same quantity; G's updated parameters are those of the fp32 CPU oracle step
    that keeps the term attached, under the bar tests/test_train_gpu.py holds the SRGAN step's parameters to
    (per tensor: L2 norm within 5e-4 of it, sum within 10 * 5e-4 of the norm)."""
    pkg = _pkg()
    res = {}
    for perceptual in (False, True):
        G, D, g_flat, d_flat, g_opt, d_opt, step = _make_step(pkg, gpu, perceptual)
        d_loss, g_loss = step(*_batch(gpu))
        res[perceptual] = (float(d_loss.detach()), float(g_loss.detach()), g_flat.data.clone(), d_flat.data.clone(), G)
    od, og, ovgg, oG = _oracle_step_with_term()
    print("d_loss %.8f / %.8f  g_loss off %.8f on %.8f oracle %.8f  term %.6f" % (res[False][0], res[True][0], res[False][1],
                                                                               res[True][1], og, ovgg))
    assert res[False][0] == res[True][0] and torch.equal(res[False][3], res[True][3])
    assert not torch.equal(res[False][2], res[True][2])
    assert abs(res[True][1] - res[False][1]) <= 2e-3 * 6e-3 * ovgg + 1e-7
    tol = 5e-4
    sd = res[True][4].state_dict()
    for n, p in oG.named_parameters():
        want = p.detach().double()
        t = sd[n].detach().double().cpu()
        l2 = float(want.pow(2).sum().sqrt())
        assert abs(float(t.pow(2).sum().sqrt()) - l2) <= tol * max(l2, 1e-8), "param L2 " + n
        assert abs(float(t.sum()) - float(want.sum())) <= 10 * tol * max(l2, 1e-8), "param sum " + n
    # ... and the oracle's update is not the one without the term (the comparison above can tell the two apart)
    sd0 = res[False][4].state_dict()
    moved = max(float((sd[n].double().cpu() - sd0[n].double().cpu()).abs().max()) for n, _ in oG.named_parameters())
    assert moved > 0


def test_step_captured_equals_eager(gpu):
    """Two replays of capture_step(step, .., flats=[g_flat, d_flat]) leave the flat parameters two eager steps leave,
    compared as tests/test_train_gpu.py compares the captured SRGAN step with the eager one (rel_err < 1e-4)."""
    pkg = _pkg()
    batches = [(fill.rand((2, 3, 8, 8), 670 + 10 * i).to(gpu), fill.rand((2, 3, 32, 32), 671 + 10 * i).to(gpu)) for i in range(2)]
    G, D, g_flat, d_flat, g_opt, d_opt, step = _make_step(pkg, gpu, True)
    ref_losses = [[float(v.detach()) for v in step(*b)] for b in batches]
    ref = (g_flat.data.clone(), d_flat.data.clone())

    G, D, g_flat, d_flat, g_opt, d_opt, step = _make_step(pkg, gpu, True)

    def state(o):
        return [o.flat.data] + [getattr(o, k) for k in ("buf", "exp_avg", "exp_avg_sq", "step_dev")
                                if getattr(o, k, None) is not None]

    snap = [[t.clone() for t in state(o)] for o in (g_opt, d_opt)]
    bn_state = [(m, m.running_mean.clone(), m.running_var.clone()) for net in (G, D) for m in net.modules()
                if isinstance(m, torch.nn.BatchNorm2d) and m.running_mean is not None]
    graphed = pkg.trainers.capture_step(step, batches[0], warmup=1, flats=[g_flat, d_flat])
    for o, saved in zip((g_opt, d_opt), snap):      # the warm-up / capture calls moved the state: restore it
        for t, t0 in zip(state(o), saved):
            t.copy_(t0)
    for m, rm, rv in bn_state:
        m.running_mean.copy_(rm)
        m.running_var.copy_(rv)
    g_flat.mark_changed()
    d_flat.mark_changed()
    got_losses = [[float(v.detach()) for v in graphed(*b)] for b in batches]
    torch.cuda.synchronize()
    print("losses eager %s graph %s; G bit-equal %s D bit-equal %s" % (ref_losses, got_losses, torch.equal(g_flat.data, ref[0]),
                                                                     torch.equal(d_flat.data, ref[1])))
    graphed.close()
    assert rel_err(np.array(got_losses), np.array(ref_losses)) < 1e-4
    assert rel_err(g_flat.data, ref[0]) < 1e-4 and rel_err(d_flat.data, ref[1]) < 1e-4


def test_step_with_pruned_dead_gradients(gpu):
    """prune_dead_grads=True with the term: the same D and G parameters after the step (the dead gradients feed nothing;
    grouped weight-gradient launches may split differently: 1e-6 of the largest parameter, as the existing test of the
    flag allows its gradients)."""
    pkg = _pkg()
    res = {}
    for prune in (False, True):
        G, D, g_flat, d_flat, g_opt, d_opt, step = _make_step(pkg, gpu, True, prune_dead_grads=prune)
        losses = [float(v.detach()) for v in step(*_batch(gpu))]
        assert all(np.isfinite(losses)) and all(p.requires_grad for p in D.parameters())
        res[prune] = (losses, g_flat.data.clone(), d_flat.data.clone())
    assert res[True][0] == res[False][0]
    for a, b in zip(res[True][1:], res[False][1:]):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


def _child(argv, timeout):
    r = subprocess.run([sys.executable] + argv, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-2000:], r.stderr[-2000:])
    return r


def test_step_data_parallel_child(gpu):
    """The step once in a fresh process under SRK_DP_FORCE_COMM=1 (a one-rank process group: both exchanges run)."""
    r = _child([os.path.join(ROOT, "tests", "perceptual_ref.py"), "dp-child"], 300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert re.search(r"dp-child d_loss \S+ g_loss \S+ ok 1", r.stdout)


def test_cli_trains_with_perceptual(gpu, tmp_path):
    """main.py --perceptual --vgg_weights <the filled head> in a child process: exit 0 and a finite G loss."""
    path = str(tmp_path / "vgg19_head.pth")
    torch.save(P.filled_head(8, 78)[2], path)
    argv = ["--model_name", "SRGAN", "--synthetic", "--perceptual", "--vgg_weights", path, "--num_epochs", "1",
            "--epoch_pretrain", "0", "--steps_per_epoch", "2", "--crop_size", "32", "--batch_size", "2",
            "--save_dir", str(tmp_path / "out")]
    r = _child([os.path.join(ROOT, "main.py")] + argv, 600)
    assert r.returncode == 0, r.stderr[-2000:]
    g = [float(m) for m in re.findall(r"Epoch: \[ *\d+\] D_loss: \S+ G_loss: (\S+)", r.stdout)]
    assert len(g) == 1 and np.isfinite(g[0]) and g[0] > 0
