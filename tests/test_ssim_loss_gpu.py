"""The SSIM training loss on the device (csrc/ssim_loss.hip: k_ssim_loss / k_ssim_loss_final; ops.ssim_loss, utils.SSIMLoss,
trainers.build(..., ssim_weight), main.py --ssim_weight) against fp64 torch autograd (tests/ssim_loss_ref.py), on the case
table that tests/test_ssim_loss_cpu.py holds the host twin to.

LOSS_TOL = 1e-6 absolute is SSIM_TOL of tests/test_ssim_gpu.py (the loss leaves the kernel as fp32).  The gradient is the
kernel's direct output and is held to the project's output contract at a tenth: max |d| <= 1e-4 * max |ref| + 1e-9.

Two cases of the issue that asked for this cannot run as it wrote them, and are mended to the nearest ones that can:
a x2 ESPCN (no padding: 5-3-3) turns 12 x 12 into 8 x 8, under the 11 x 11 window, so the oracle step feeds 14 x 14 (the
smallest that leaves a window, 12 x 12), and 12 x 12 is checked to raise; the command line gets --scale_factor 2, because
with the default x4 a crop of 32 leaves ESPCN an empty output with or without the loss."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import assert_close_elementwise
from oracle import fill, ref_modules as M
import ssim_loss_ref as L

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-6
GRAD_RTOL, GRAD_ATOL = 1e-4, 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _tile():
    """(kLossTH, kLossTW, kLossMaxPlanes) as the kernel source states them."""
    with open(os.path.join(ROOT, "pytorch_super_resolution_model_collection_amd", "csrc", "ssim_loss.hip")) as f:
        text = f.read()
    th, tw = re.search(r"constexpr int kLossTH = (\d+), kLossTW = (\d+);", text).groups()
    return int(th), int(tw), int(re.search(r"constexpr int kLossMaxPlanes = (\d+);", text).group(1))


def laid_out(a, layout, gpu):
    """The fp32 [N,C,H,W] array on the device with the strides of `layout` (test_ssim_gpu.laid_out)."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    if layout == 'nchw':
        return t.contiguous()
    if layout == 'channels_last':
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    big = torch.full((a.shape[0], a.shape[1], a.shape[2] + 5, a.shape[3] + 9), 7.0, device=gpu)
    big[:, :, 2:2 + a.shape[2], 6:6 + a.shape[3]] = t
    return big[:, :, 2:2 + a.shape[2], 6:6 + a.shape[3]]


def device_loss(pd, gd, grad=True):
    """ops.ssim_loss forward (+ backward): (loss 0-dim device tensor, d loss / d pred device tensor or None)."""
    pkg = _pkg()
    x = pd.detach().requires_grad_(grad)
    loss = pkg.ops.ssim_loss(x, gd)
    assert loss.dim() == 0 and loss.is_cuda and loss.dtype == torch.float32
    if not grad:
        return loss.detach(), None
    pkg.ops.backward(loss)
    return loss.detach(), x.grad


def check(name, p, g, gpu, want=None):
    want_loss, want_grad = want if want is not None else L.loss_and_grad(p, g)
    loss, grad = device_loss(torch.from_numpy(p).to(gpu), torch.from_numpy(g).to(gpu))
    err = float(np.abs(grad.cpu().numpy().astype(np.float64) - want_grad).max())
    bar = GRAD_RTOL * float(np.abs(want_grad).max()) + GRAD_ATOL
    print("%-28s loss %.9f (fp64 %.9f, off by %.2e)  gradient: worst |d| %.3e, max |ref| %.3e, %.3g of the bar"
          % (name, float(loss), want_loss, abs(float(loss) - want_loss), err, np.abs(want_grad).max(), err / bar))
    assert abs(float(loss) - want_loss) <= LOSS_TOL, (name, float(loss), want_loss)
    assert err <= bar, (name, err, bar)
    return loss, grad


@pytest.mark.parametrize("name", sorted(L.cases()))
def test_table_against_fp64(gpu, name):
    p, g = L.cases()[name]
    loss, grad = check(name, p, g, gpu, L.reference(name))
    if name == "batch_rgb":      # pred is read unclamped: the pixels outside [0, 1] keep their gradient
        out = torch.from_numpy(L.out_of_range(p)).to(gpu)
        assert int(out.sum()) > 100 and bool((grad[out] != 0).all())
    if name == "identical":
        assert abs(float(loss)) <= 1e-7


def _shapes():
    th, tw, mp = _tile()
    return [(1, 1, 11, 11),                      # one position
            (1, 1, 11, 300), (1, 1, 300, 11),    # one row / one column of positions
            (1, 2, 2 * th + 1, 3 * tw + 1),      # the last tile holds exactly one pixel in each direction
            (1, 1, th + 11, tw + 11),            # ... and the last tile of positions exactly one position
            (2, 1, 2 * th, 3 * tw),              # exact multiples of the tile
            (1, 1, 97, 131),
            (2, 3, 23, 37),                      # N = 2 with C = 3
            (1, mp + 1, 20, 23),                 # the plane grouping wraps: a group of mp planes and one of 1
            (2, 2 * mp + 1, 13, 29)]


@pytest.mark.parametrize("shape", _shapes(), ids=lambda s: "x".join(str(v) for v in s))
def test_tile_edges_and_plane_groups_against_fp64(gpu, shape):
    rng = np.random.RandomState(sum(shape))
    g = rng.rand(*shape).astype(np.float32)
    p = (g + 0.1 * rng.randn(*shape)).astype(np.float32)
    check(str(shape), p, g, gpu)


def test_layouts_give_the_same_bits(gpu):
    """pred NCHW-contiguous or channels_last, target NCHW, channels_last or a cropped strided view: one result."""
    p, g = L.cases()["batch_rgb"]
    base_loss, base_grad = device_loss(laid_out(p, 'channels_last', gpu), laid_out(g, 'channels_last', gpu))
    for pl in ('nchw', 'channels_last'):
        for gl in ('nchw', 'channels_last', 'cropped_view'):
            loss, grad = device_loss(laid_out(p, pl, gpu), laid_out(g, gl, gpu))
            assert torch.equal(loss, base_loss) and torch.equal(grad, base_grad), (pl, gl)


def test_determinism_and_paths(gpu, monkeypatch):
    pkg = _pkg()
    p, g = L.cases()["batch_rgb"]
    pd, gd = torch.from_numpy(p).to(gpu), torch.from_numpy(g).to(gpu)
    loss, grad = device_loss(pd, gd)
    loss2, grad2 = device_loss(pd, gd)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)              # no atomics: the same bits
    assert torch.equal(device_loss(pd, gd, grad=False)[0], loss)              # loss only: the same loss
    assert torch.equal(pkg.utils.SSIMLoss()(pd, torch.from_numpy(g)), loss)   # the module; a CPU target is moved over

    lib = pkg._lib.load()
    calls = []
    real = lib.srk_scale_dev
    monkeypatch.setattr(lib, "srk_scale_dev", lambda *a: calls.append(1) or real(*a))
    # the declared seed is folded into the gradient by the loss kernel; the backward hands it out as it is
    seed = torch.full((), 0.25, device=gpu)
    x = pd.clone().requires_grad_(True)
    with pkg.ops.loss_seed(0.25, seed):
        seeded = pkg.ops.ssim_loss(x, gd)
    pkg.ops.backward(seeded, seed)
    assert not calls and torch.equal(seeded.detach(), loss)
    want = 0.25 * grad
    ulp = torch.maximum((torch.nextafter(want, torch.full_like(want, float('inf'))) - want).abs(),
                        (want - torch.nextafter(want, torch.full_like(want, float('-inf')))).abs())
    assert bool(((x.grad - want).abs() <= ulp).all())
    # the unit seed: as it is, no launch
    x = pd.clone().requires_grad_(True)
    pkg.ops.backward(pkg.ops.ssim_loss(x, gd))
    assert not calls and torch.equal(x.grad, grad)
    # a foreign upstream gradient takes srk_scale_dev
    x = pd.clone().requires_grad_(True)
    pkg.ops.ssim_loss(x, gd).backward(torch.full((), 3.0, device=gpu))
    assert len(calls) == 1
    assert float((x.grad - 3.0 * grad).abs().max()) <= 3e-7 * float(grad.abs().max())   # one fp32 product per element
    # it composes with loss_sum
    x = pd.clone().requires_grad_(True)
    mix = pkg.ops.loss_sum(pkg.ops.mse_loss(x, gd), pkg.ops.ssim_loss(x, gd), 0.7, 0.3)
    pkg.ops.backward(mix)
    xm = pd.clone().requires_grad_(True)
    mse = pkg.ops.mse_loss(xm, gd)
    pkg.ops.backward(mse)
    # (fp32 on both sides, a handful of roundings of 6e-8 each on values below 1 / on the larger of the two terms)
    assert abs(float(mix) - (0.7 * float(mse) + 0.3 * float(loss))) <= 1e-6
    want = 0.7 * xm.grad + 0.3 * grad
    assert float((x.grad - want).abs().max()) <= 1e-6 * max(float(xm.grad.abs().max()), float(grad.abs().max()))


def test_small_planes_are_refused_by_name(gpu):
    pkg = _pkg()
    for shape in ((1, 1, 10, 40), (2, 3, 32, 8)):
        t = torch.rand(shape, device=gpu)
        with pytest.raises(RuntimeError, match=re.escape(str(tuple(shape)))):
            pkg.ops.ssim_loss(t, t)
    with pytest.raises(RuntimeError):
        pkg.ops.ssim_loss(torch.rand(4, 200, device=gpu), torch.rand(4, 200, device=gpu))


def _grads(net):
    return {n: p.grad.detach().cpu() for n, p in net.named_parameters()}


def _oracle_grads(ora, losses):
    """Gradients of the fp64 oracle under every name of its state_dict (shared parameters appear under each of theirs)."""
    ora.zero_grad()
    for l in losses:
        l.backward(retain_graph=True)
    return {n: p.grad.detach().float() for n, p in ora.state_dict(keep_vars=True).items() if p.requires_grad}


def test_espcn_step_gradients_against_the_oracle(gpu, monkeypatch):
    """fwd_bwd of build('espcn', ..., ssim_weight=0.3) against oracle.ref_modules' net in fp64 under the reference mix.
    On one GPU both loss kernels fold their weight into the gradient: no srk_scale_dev pass in the step."""
    pkg = _pkg()
    lib, scale_calls = pkg._lib.load(), []
    real = lib.srk_scale_dev
    monkeypatch.setattr(lib, "srk_scale_dev", lambda *a: scale_calls.append(1) or real(*a))
    a = 0.3
    net, ora = pkg.ESPCNNet(1, 64, 2), M.ESPCN(1, 64, 2)
    fill.fill_module(ora, 7, 1.0)
    net.load_state_dict(ora.state_dict())
    net.to(gpu).train()
    ora.double()
    x, t = fill.rand((2, 1, 14, 14), 201), fill.rand((2, 1, 12, 12), 202)
    flat, opt, dp, step = pkg.trainers.build("espcn", net, 1e-3, ssim_weight=a)
    loss = step.segments[0][0](x.to(gpu), t.to(gpu))
    mse = lambda p, q: ((p - q) ** 2).mean()
    ref = L.mix_loss(mse, a)(ora(x.double()), t.double())
    want = _oracle_grads(ora, [ref])
    print("espcn mix loss %.9f (fp64 %.9f)" % (float(loss), float(ref)))
    assert not scale_calls
    assert abs(float(loss) - float(ref)) <= 1e-3 * abs(float(ref))      # the output contract
    for n, g in _grads(net).items():
        assert_close_elementwise(g, want[n], 1e-3, what="espcn ssim_weight %.1f d %s" % (a, n))
    # the stated 12 x 12 input leaves 8 x 8, under the window: refused by name
    with pytest.raises(RuntimeError, match=re.escape("(2, 1, 8, 8)")):
        step.segments[0][0](fill.rand((2, 1, 12, 12), 203).to(gpu), fill.rand((2, 1, 8, 8), 204).to(gpu))


def test_lapsrn_step_gradients_against_the_oracle(gpu):
    """lapsrn_step with ssim_weight: the same mix on both levels, two backward passes into the same gradients."""
    pkg = _pkg()
    a = 0.3
    net, ora = pkg.LapSRNNet(1, 64, 3), M.LapSRN(1, 64, 3)
    fill.fill_module(ora, 9, 1.0)
    net.load_state_dict(ora.state_dict())
    net.to(gpu).train()
    ora.double()
    x, t2, t4 = fill.rand((2, 1, 8, 8), 211), fill.rand((2, 1, 16, 16), 212), fill.rand((2, 1, 32, 32), 213)
    flat, opt, dp, step = pkg.trainers.build("lapsrn", net, 0.0, ssim_weight=a)     # lr 0: the step leaves the gradients to read
    before = flat.data.clone()
    l1, l2 = step(x.to(gpu), t2.to(gpu), t4.to(gpu))
    assert torch.equal(flat.data, before)
    mix = L.mix_loss(M.L1_Charbonnier_loss(), a)
    hr2, hr4 = ora(x.double())
    r1, r2 = mix(hr2, t2.double()), mix(hr4, t4.double())
    want = _oracle_grads(ora, [r1, r2])
    print("lapsrn mix losses %.9f %.9f (fp64 %.9f %.9f)" % (float(l1), float(l2), float(r1), float(r2)))
    assert abs(float(l1) - float(r1)) <= 1e-3 * abs(float(r1)) and abs(float(l2) - float(r2)) <= 1e-3 * abs(float(r2))
    for n, g in _grads(net).items():
        assert_close_elementwise(g, want[n], 1e-3, what="lapsrn ssim_weight %.1f d %s" % (a, n))


def test_weight_zero_is_the_step_of_today(gpu, monkeypatch):
    """build(kind, ..., ssim_weight=0.0) hands loss_segments the very object ops.mse_loss / ops.l1_loss."""
    pkg = _pkg()
    seen = []
    real = pkg.trainers.loss_segments
    monkeypatch.setattr(pkg.trainers, "loss_segments", lambda model, opt, loss_fn, *a, **k: seen.append(loss_fn) or real(model, opt, loss_fn, *a, **k))
    nets = {"srcnn": lambda: pkg.SRCNNNet(1, 64), "fsrcnn": lambda: pkg.FSRCNNNet(1, 2, 56, 12, 4),
            "espcn": lambda: pkg.ESPCNNet(1, 64, 2), "vdsr": lambda: pkg.VDSRNet(1, 64, 2), "edsr": lambda: pkg.EDSRNet(1, 64, 2)}
    for kind, make in nets.items():
        want = pkg.ops.l1_loss if kind == "edsr" else pkg.ops.mse_loss
        for kw in ({}, {"ssim_weight": 0.0}):
            pkg.trainers.build(kind, make().to(gpu), 1e-3, **kw)
            assert seen.pop() is want, (kind, kw)
        pkg.trainers.build(kind, make().to(gpu), 1e-3, ssim_weight=0.25)
        assert seen.pop() is not want
    assert pkg.trainers.mixed_loss(pkg.ops.charbonnier_loss, 0.0) is pkg.ops.charbonnier_loss
    with pytest.raises(ValueError):
        pkg.trainers.build("edsr", nets["edsr"]().to(gpu), 1e-3, ssim_weight=1.5)


def test_captured_step_equals_eager(gpu):
    """Three steps through AutoGraph (one eager, the capture, two replays) and three eager steps from the same
    parameters: the same loss bits and the same parameter bits."""
    pkg = _pkg()
    batches = [(fill.rand((2, 1, 16, 16), 220 + i).to(gpu), fill.rand((2, 1, 16, 16), 230 + i).to(gpu)) for i in range(3)]
    res = {}
    for mode in ("eager", "graph"):
        net = pkg.ESPCNNet(1, 64, 2)
        fill.fill_module(net, 5, 1.0)
        net.to(gpu).train()
        flat, opt, dp, step = pkg.trainers.build("espcn", net, 1e-2, ssim_weight=0.3)
        run = step
        if mode == "graph":
            run = pkg.trainers.AutoGraph(step, lambda ts: pkg.trainers.capture_step(step, ts, warmup=0, flats=[flat]))
        losses = [run(*b).clone() for b in batches]
        if mode == "graph":
            assert run.graph is not None
            run.close()
        res[mode] = (torch.stack(losses).cpu(), flat.data.detach().cpu().clone())
    print("losses eager %s graph %s" % (res["eager"][0].tolist(), res["graph"][0].tolist()))
    assert torch.equal(res["eager"][0], res["graph"][0])
    assert torch.equal(res["eager"][1], res["graph"][1])


def test_cli_trains_with_ssim_weight(gpu, tmp_path):
    """main.py --ssim_weight 0.2 in a child process: exit 0 and a finite (mixed) loss per epoch."""
    argv = ["--model_name", "ESPCN", "--synthetic", "--num_epochs", "1", "--steps_per_epoch", "2", "--num_channels", "1",
            "--crop_size", "32", "--batch_size", "2", "--ssim_weight", "0.2", "--scale_factor", "2", "--save_dir", str(tmp_path)]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + argv, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [float(m) for m in re.findall(r"Epoch: \[ *\d+\] avg loss: (\S+)", r.stdout)]
    assert len(losses) == 1 and all(np.isfinite(losses)) and 0 < losses[0] < 2
