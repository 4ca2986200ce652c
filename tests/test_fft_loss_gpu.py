"""The frequency-domain loss on the device (csrc/fft_loss.hip: k_fft_diff / k_fft_rows / k_fft_cols / k_fft_grad /
k_fft_final; ops.fft_loss, utils.FFTLoss, trainers.build(..., fft_weight), main.py --fft_weight) against the fp64
restatement (tests/fft_loss_ref.py), on the case table that tests/test_fft_loss_cpu.py holds the host twin to.

The bars are the project's for a loss kernel: the loss, which leaves the kernel as fp32, within
1e-6 * max(1, |ref|); the gradient, the kernel's direct output, within 1e-4 * max |ref| + 1e-9.  The sign is
discontinuous; tests/test_fft_loss_cpu.py asserts on the reference alone that no free bin of any case lies within
1e-9 * max |F| of zero, far above what an fp64 DFT of these sizes is off by, so a flipped sign here is a wrong kernel."""
import numpy as np
import pytest
import torch

from conftest import assert_close_elementwise
from oracle import fill, ref_modules as M
import fft_loss_ref as L
import ssim_loss_ref as SL

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-6
GRAD_RTOL, GRAD_ATOL = 1e-4, 1e-9


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def laid_out(a, layout, gpu):
    """The fp32 [N,C,H,W] array on the device with the strides of `layout`."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    if layout == 'nchw':
        return t.contiguous()
    if layout == 'channels_last':
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    big = torch.full((a.shape[0], a.shape[1], a.shape[2] + 5, a.shape[3] + 9), 7.0, device=gpu)
    big[:, :, 2:2 + a.shape[2], 6:6 + a.shape[3]] = t
    return big[:, :, 2:2 + a.shape[2], 6:6 + a.shape[3]]


def device_loss(pd, gd, norm="backward", grad=True):
    """ops.fft_loss forward (+ backward): (loss 0-dim device tensor, d loss / d pred device tensor or None)."""
    pkg = _pkg()
    x = pd.detach().requires_grad_(grad)
    loss = pkg.ops.fft_loss(x, gd, norm)
    assert loss.dim() == 0 and loss.is_cuda and loss.dtype == torch.float32
    if not grad:
        return loss.detach(), None
    pkg.ops.backward(loss)
    return loss.detach(), x.grad


@pytest.mark.parametrize("name", sorted(L.cases()))
def test_table_against_fp64(gpu, name):
    p, g, norm = L.cases()[name]
    want_loss, want_grad = L.reference(name)
    loss, grad = device_loss(torch.from_numpy(p).to(gpu), torch.from_numpy(g).to(gpu), norm)
    assert grad.shape == p.shape
    err = float(np.abs(grad.cpu().numpy().astype(np.float64) - want_grad).max())
    bar = GRAD_RTOL * float(np.abs(want_grad).max()) + GRAD_ATOL
    lbar = LOSS_TOL * max(1.0, abs(want_loss))
    print("%-22s loss %.9f (fp64 %.9f, off by %.2e, %.3g of the bar)  gradient: worst |d| %.3e, max |ref| %.3e, %.3g of the bar"
          % (name, float(loss), want_loss, abs(float(loss) - want_loss), abs(float(loss) - want_loss) / lbar, err,
             np.abs(want_grad).max(), err / bar))
    assert abs(float(loss) - want_loss) <= lbar, (name, float(loss), want_loss)
    assert err <= bar, (name, err, bar)
    if name == "identical":
        assert float(loss) == 0.0 and not bool(grad.any())      # exact zeros, both


def test_determinism_and_paths(gpu, monkeypatch):
    pkg = _pkg()
    p, g, _ = L.cases()["12_1x2x130x66"]
    pd, gd = torch.from_numpy(p).to(gpu), torch.from_numpy(g).to(gpu)
    loss, grad = device_loss(pd, gd)
    loss2, grad2 = device_loss(pd, gd)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)              # no atomics: the same bits
    assert torch.equal(device_loss(pd, gd, grad=False)[0], loss)              # loss only: the same loss
    assert torch.equal(pkg.utils.FFTLoss()(pd, torch.from_numpy(g)), loss)    # the module; a CPU target is moved over
    want = L.loss_and_grad(p, g, "ortho")[0]
    assert abs(float(pkg.utils.FFTLoss("ortho")(pd, gd)) - want) <= LOSS_TOL * max(1.0, want)

    lib = pkg._lib.load()
    calls = []
    real = lib.srk_scale_dev
    monkeypatch.setattr(lib, "srk_scale_dev", lambda *a: calls.append(1) or real(*a))
    near = lambda got, want: bool(((got - want).abs() <= 2e-7 * want.abs() + 1e-30).all())   # two fp32 roundings against one
    # the declared seed is folded into the gradient by the kernel; the backward hands it out as it is
    seed = torch.full((), 0.25, device=gpu)
    x = pd.clone().requires_grad_(True)
    with pkg.ops.loss_seed(0.25, seed):
        seeded = pkg.ops.fft_loss(x, gd)
    pkg.ops.backward(seeded, seed)
    assert not calls and torch.equal(seeded.detach(), loss) and near(x.grad, 0.25 * grad)
    # the unit seed: as it is, no launch
    x = pd.clone().requires_grad_(True)
    pkg.ops.backward(pkg.ops.fft_loss(x, gd))
    assert not calls and torch.equal(x.grad, grad)
    # weighted_term folds its weight the same way (the seed is the constant loss_sum's backward hands out) ...
    fft = lambda a, b: pkg.ops.fft_loss(a, b, "backward")
    x = pd.clone().requires_grad_(True)
    xm = pd.clone().requires_grad_(True)
    mix = pkg.ops.loss_sum(pkg.ops.mse_loss(xm, gd), pkg.ops.weighted_term(fft, 0.1, x, gd), 1.0, 0.1)
    pkg.ops.backward(mix)
    assert not calls
    folded = x.grad.clone()
    # ... and the general path, a foreign upstream gradient, takes srk_scale_dev over the unweighted gradient
    x = pd.clone().requires_grad_(True)
    pkg.ops.fft_loss(x, gd).backward(torch.full((), 0.1, device=gpu))
    assert len(calls) == 1
    assert near(folded, x.grad) and near(folded, 0.1 * grad)
    xp = pd.clone().requires_grad_(True)
    pkg.ops.backward(pkg.ops.mse_loss(xp, gd))
    assert torch.equal(xm.grad, xp.grad)
    assert abs(float(mix) - (float(pkg.ops.mse_loss(pd, gd)) + 0.1 * float(loss))) <= 1e-6 * max(1.0, float(loss))
    # no gradient where pred needs none, none to the target
    assert not pkg.ops.fft_loss(pd, gd).requires_grad
    t = gd.clone().requires_grad_(True)
    out = pkg.ops.fft_loss(pd, t)
    pkg.ops.backward(out)
    assert torch.equal(out.detach(), loss) and t.grad is None


def test_a_nan_poisons_its_plane_only(gpu):
    p, g, _ = [a.copy() if isinstance(a, np.ndarray) else a for a in L.cases()["07_2x5x16x16"]]
    p[1, 3, 5, 6] = np.nan
    loss, grad = device_loss(torch.from_numpy(p).to(gpu), torch.from_numpy(g).to(gpu))
    assert bool(torch.isnan(loss)) and bool(torch.isnan(grad[1, 3]).all())
    clean = L.reference("07_2x5x16x16")[1].copy()
    got = grad.cpu().numpy().astype(np.float64)
    got[1, 3] = clean[1, 3]
    assert np.isfinite(got).all() and np.abs(got - clean).max() <= GRAD_RTOL * np.abs(clean).max() + GRAD_ATOL


def test_layouts_give_the_same_bits(gpu):
    """pred NCHW-contiguous or channels_last, target NCHW, channels_last or a cropped strided view: one result."""
    p, g, _ = L.cases()["08_1x3x17x33"]
    base_loss, base_grad = device_loss(laid_out(p, 'channels_last', gpu), laid_out(g, 'channels_last', gpu))
    for pl in ('nchw', 'channels_last'):
        for gl in ('nchw', 'channels_last', 'cropped_view'):
            loss, grad = device_loss(laid_out(p, pl, gpu), laid_out(g, gl, gpu))
            assert torch.equal(loss, base_loss) and torch.equal(grad, base_grad), (pl, gl)


def test_large_planes_are_refused_by_name(gpu):
    pkg = _pkg()
    for shape in ((1, 1, 257, 8), (1, 2, 8, 300)):
        t = torch.zeros(shape, device=gpu)
        with pytest.raises(RuntimeError, match="%d x %d.*256" % shape[2:]):
            pkg.ops.fft_loss(t, t)
    with pytest.raises(RuntimeError):
        pkg.ops.fft_loss(torch.rand(4, 200, device=gpu), torch.rand(4, 200, device=gpu))


def _grads(net):
    return {n: p.grad.detach().cpu() for n, p in net.named_parameters()}


def _oracle_grads(ora, losses):
    """Gradients of the fp64 oracle under every name of its state_dict (shared parameters appear under each of theirs)."""
    ora.zero_grad()
    for l in losses:
        l.backward(retain_graph=True)
    return {n: p.grad.detach().float() for n, p in ora.state_dict(keep_vars=True).items() if p.requires_grad}


def test_espcn_step_gradients_against_the_oracle(gpu, monkeypatch):
    """fwd_bwd of build('espcn', ..., fft_weight=0.1) against oracle.ref_modules' net in fp64 under mse + 0.1 * FFT.
    On one GPU the loss kernel folds the weight into its gradient: no srk_scale_dev pass in the step."""
    pkg = _pkg()
    lib, scale_calls = pkg._lib.load(), []
    real = lib.srk_scale_dev
    monkeypatch.setattr(lib, "srk_scale_dev", lambda *a: scale_calls.append(1) or real(*a))
    w = 0.1
    net, ora = pkg.ESPCNNet(1, 64, 2), M.ESPCN(1, 64, 2)
    fill.fill_module(ora, 7, 1.0)
    net.load_state_dict(ora.state_dict())
    net.to(gpu).train()
    ora.double()
    x, t = fill.rand((2, 1, 14, 14), 301), fill.rand((2, 1, 12, 12), 302)
    flat, opt, dp, step = pkg.trainers.build("espcn", net, 1e-3, fft_weight=w)
    loss = step.segments[0][0](x.to(gpu), t.to(gpu))
    mse = lambda p, q: ((p - q) ** 2).mean()
    ref = L.mix_loss(mse, w)(ora(x.double()), t.double())
    want = _oracle_grads(ora, [ref])
    print("espcn mse + %.1f fft: loss %.9f (fp64 %.9f)" % (w, float(loss), float(ref)))
    assert not scale_calls
    assert abs(float(loss) - float(ref)) <= 1e-3 * abs(float(ref))      # the output contract
    for n, g in _grads(net).items():
        assert_close_elementwise(g, want[n], 1e-3, what="espcn fft_weight %.1f d %s" % (w, n))


def test_lapsrn_step_gradients_against_the_oracle(gpu):
    """lapsrn_step with all three terms, [(1 - a) Charbonnier + a (1 - SSIM)] + w FFT("ortho"), on both levels."""
    pkg = _pkg()
    a, w = 0.3, 0.1
    net, ora = pkg.LapSRNNet(1, 64, 3), M.LapSRN(1, 64, 3)
    fill.fill_module(ora, 9, 1.0)
    net.load_state_dict(ora.state_dict())
    net.to(gpu).train()
    ora.double()
    x, t2, t4 = fill.rand((2, 1, 8, 8), 311), fill.rand((2, 1, 16, 16), 312), fill.rand((2, 1, 32, 32), 313)
    flat, opt, dp, step = pkg.trainers.build("lapsrn", net, 0.0, ssim_weight=a, fft_weight=w, fft_norm="ortho")   # lr 0
    before = flat.data.clone()
    l1, l2 = step(x.to(gpu), t2.to(gpu), t4.to(gpu))
    assert torch.equal(flat.data, before)
    mix = L.mix_loss(SL.mix_loss(M.L1_Charbonnier_loss(), a), w, "ortho")
    hr2, hr4 = ora(x.double())
    r1, r2 = mix(hr2, t2.double()), mix(hr4, t4.double())
    want = _oracle_grads(ora, [r1, r2])
    print("lapsrn three-term losses %.9f %.9f (fp64 %.9f %.9f)" % (float(l1), float(l2), float(r1), float(r2)))
    assert abs(float(l1) - float(r1)) <= 1e-3 * abs(float(r1)) and abs(float(l2) - float(r2)) <= 1e-3 * abs(float(r2))
    for n, g in _grads(net).items():
        assert_close_elementwise(g, want[n], 1e-3, what="lapsrn ssim %.1f fft %.1f d %s" % (a, w, n))


def test_weight_zero_is_the_step_of_today(gpu, monkeypatch):
    """build(kind, ..., fft_weight=0.0) hands loss_segments the very object ops.mse_loss / ops.l1_loss, and an EDSR step
    built with fft_weight=0 leaves the same bits as one built without the argument."""
    pkg = _pkg()
    seen = []
    real = pkg.trainers.loss_segments
    monkeypatch.setattr(pkg.trainers, "loss_segments", lambda model, opt, loss_fn, *a, **k: seen.append(loss_fn) or real(model, opt, loss_fn, *a, **k))
    res = []
    x, t = fill.rand((2, 1, 8, 8), 321).to(gpu), fill.rand((2, 1, 32, 32), 322).to(gpu)
    for kw in ({}, {"fft_weight": 0.0, "fft_norm": "ortho"}, {"fft_weight": 0.05}):
        net = pkg.EDSRNet(1, 64, 2)
        fill.fill_module(net, 5, 1.0)
        net.to(gpu).train()
        flat, opt, dp, step = pkg.trainers.build("edsr", net, 1e-3, **kw)
        assert (seen.pop() is pkg.ops.l1_loss) == (kw.get("fft_weight", 0.0) == 0.0)
        loss = step(x, t)
        res.append((loss.detach().clone(), flat.data.detach().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][1], res[2][1]) and float(res[2][0]) > float(res[0][0])
    with pytest.raises(ValueError):
        pkg.trainers.build("edsr", pkg.EDSRNet(1, 64, 2).to(gpu), 1e-3, fft_weight=-1.0)


def test_captured_step_equals_eager(gpu):
    """Three ESPCN x2 steps with fft_weight=0.1 through AutoGraph (one eager, the capture, a replay) and three eager steps
    from the same parameters: the same loss bits and the same parameter bits."""
    pkg = _pkg()
    batches = [(fill.rand((2, 1, 16, 16), 330 + i).to(gpu), fill.rand((2, 1, 16, 16), 340 + i).to(gpu)) for i in range(3)]
    res = {}
    for mode in ("eager", "graph"):
        net = pkg.ESPCNNet(1, 64, 2)
        fill.fill_module(net, 5, 1.0)
        net.to(gpu).train()
        flat, opt, dp, step = pkg.trainers.build("espcn", net, 1e-2, fft_weight=0.1)
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
