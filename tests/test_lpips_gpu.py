"""LPIPS on the device (csrc/lpips.hip: k_lpips / k_lpips_row / k_lpips_finish; ops.lpips_layer, ops.lpips, models.LPIPS,
trainers.mixed_loss(lpips_weight=), test()) against the fp64 restatement of tests/lpips_ref.py.

Bars (lpips_ref): the layer op is fp64 inside and is held to the plain contract, 1e-4 * max|ref| for values and
1e-3 * max|ref| for gradients -- and, because a planted all-zero pixel of f0 carries a gradient of order 1 / 1e-10 that
would hide everything else under such a bar, the gradient of the other pixels to the same contract on their own maximum.
The whole metric runs through fp32 ReLU and pool decisions: perceptual_ref.bar's rule, the contract or twice torch's own
fp32 CPU error against fp64, whichever is larger; both numbers are printed (profiles/lpips_parity.txt).
The train steps are held to an fp32 CPU oracle step that keeps the term, at test_train_gpu's bar for updated parameters.
EDSRNet upsamples by 4 whatever the scale (two 2x stages, as the reference), so its step runs LR 4 x 4 -> HR 16 x 16."""
import numpy as np
import pytest
import torch

import lpips_ref as R
from oracle import fill, ref_modules as M

pytestmark = pytest.mark.gpu
CL = torch.channels_last
PARAM_TOL = 2e-4      # tests/test_train_gpu.py: TOL of _check_params


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def run_layer(gpu, f0, f1, w, g, fmt=CL, rows=3, row=1):
    """(value [N] fp64, df0 [N,C,H,W] fp32, the table) of ops.lpips_layer on the device."""
    pkg = _pkg()
    a = f0.to(gpu).contiguous(memory_format=fmt).requires_grad_(True)
    b = f1.to(gpu).contiguous(memory_format=fmt)
    table = torch.zeros((rows, f0.shape[0]), dtype=torch.float64, device=gpu)
    value = pkg.ops.lpips_layer(a, b, w.to(gpu), row, table)
    value.backward(g.to(gpu))
    return value.detach().clone(), a.grad.detach().clone(), table


@pytest.mark.parametrize("shape", R.LAYER_SHAPES, ids=_ids(R.LAYER_SHAPES))
def test_layer_value_and_gradient(gpu, shape):
    case = R.layer_case(shape)
    value, df0, table = run_layer(gpu, case["f0"], case["f1"], case["w"], case["g"])
    assert torch.equal(table[1], value) and float(table[0].abs().max()) == 0.0 and float(table[2].abs().max()) == 0.0
    ve, vs = R.max_err(value, case["value"])
    ge, gs = R.max_err(df0, case["df0"])
    live = (case["f0"].abs().sum(1, keepdim=True) > 0).expand_as(case["f0"])     # pixels whose f0 is not all zero
    le, ls = (R.max_err(df0.cpu()[live], case["df0"][live]) if bool(live.any()) else (0.0, 0.0))
    print("lpips_layer %-14s value err %.3g of %.3g  grad err %.3g of %.3g  (non-zero pixels %.3g of %.3g)"
          % (shape, ve, vs, ge, gs, le, ls))
    assert ve <= R.OUT_CONTRACT * vs and ge <= R.GRAD_CONTRACT * gs and le <= R.GRAD_CONTRACT * ls
    assert bool(torch.isfinite(df0).all())
    again = run_layer(gpu, case["f0"], case["f1"], case["w"], case["g"])
    assert torch.equal(again[0], value) and torch.equal(again[1], df0)          # two calls: the same bits


def test_layer_layouts_and_alignment(gpu):
    """An NCHW-dense input goes through the layout kernel to the same bits; maps at an odd float offset take the 4-byte path
    (C % 4 == 0 notwithstanding) to the same numbers within the contract."""
    shape = (2, 5, 7, 70)
    case = R.layer_case(shape)
    base = run_layer(gpu, case["f0"], case["f1"], case["w"], case["g"])
    nchw = run_layer(gpu, case["f0"], case["f1"], case["w"], case["g"], fmt=torch.contiguous_format)
    assert torch.equal(nchw[0], base[0]) and torch.equal(nchw[1], base[1])
    pkg = _pkg()
    case = R.layer_case((1, 9, 8, 64))
    want_v, want_g, _ = run_layer(gpu, case["f0"], case["f1"], case["w"], case["g"])

    def shifted(t):      # the same NHWC values one float past a 16-byte boundary
        n, c, h, w = t.shape
        flat = torch.zeros(t.numel() + 1, device=gpu)
        flat[1:] = t.permute(0, 2, 3, 1).reshape(-1).to(gpu)
        v = flat[1:].view(n, h, w, c).permute(0, 3, 1, 2)
        assert v.data_ptr() % 16 == 4
        return v
    a = shifted(case["f0"]).requires_grad_(True)
    table = torch.zeros((1, 1), dtype=torch.float64, device=gpu)
    value = pkg.ops.lpips_layer(a, shifted(case["f1"]), case["w"].to(gpu), 0, table)
    value.backward(case["g"].to(gpu))
    ve, vs = R.max_err(value, want_v)
    ge, gs = R.max_err(a.grad, want_g)
    print("unaligned maps: value err %.3g of %.3g, grad err %.3g of %.3g" % (ve, vs, ge, gs))
    assert ve <= R.OUT_CONTRACT * vs and ge <= R.GRAD_CONTRACT * gs


def test_layer_of_one_tensor_is_exactly_zero(gpu):
    pkg = _pkg()
    for shape in ((2, 5, 7, 70), (1, 9, 8, 64), (1, 3, 3, 512)):
        case = R.layer_case(shape)
        f = case["f0"].to(gpu).contiguous(memory_format=CL).requires_grad_(True)
        table = torch.ones((1, shape[0]), dtype=torch.float64, device=gpu)
        value = pkg.ops.lpips_layer(f, f, case["w"].to(gpu), 0, table)
        value.backward(torch.ones(shape[0], dtype=torch.float64, device=gpu))
        assert float(value.detach().abs().max()) == 0.0 and float(f.grad.abs().max()) == 0.0, shape


def test_layer_arguments(gpu):
    pkg = _pkg()
    f = torch.zeros(1, 4, 2, 2, device=gpu)
    w = torch.ones(4, device=gpu)
    table = torch.zeros((2, 1), dtype=torch.float64, device=gpu)
    for args in ((f, f[:, :2], w, 0, table), (f, f, w[:3], 0, table), (f, f, w, 2, table), (f, f, w, 0, table.float()),
                 (f, f, w, 0, torch.zeros((2, 3), dtype=torch.float64, device=gpu))):
        with pytest.raises(RuntimeError):
            pkg.ops.lpips_layer(*args)


# -- the whole metric ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(gpu):
    _, _, _, vgg_sd, lin_sd = R.filled_net()
    return _pkg().LPIPS(vgg_sd, lin_sd).to(gpu).eval()


@pytest.mark.parametrize("normalize", (True, False))
@pytest.mark.parametrize("shape", R.METRIC_SHAPES, ids=_ids(R.METRIC_SHAPES))
def test_metric_values_and_gradient(gpu, net, shape, normalize):
    pkg = _pkg()
    case = R.metric_case(shape, normalize)
    pred = case["pred"].to(gpu).requires_grad_(True)
    target = case["target"].to(gpu).requires_grad_(True)
    values = pkg.ops.lpips(pred.detach(), target.detach(), net, normalize, reduce=False)
    assert tuple(values.shape) == (shape[0],) and values.dtype == torch.float32 and not values.requires_grad
    loss = pkg.ops.lpips(pred, target, net, normalize)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    pkg.ops.backward(loss)
    ve, vs = R.max_err(values, case["v64"])
    ge, gs = R.max_err(pred.grad, case["d64"])
    vbar, gbar = R.bar(R.OUT_CONTRACT, case["v_err32"], vs), R.bar(R.GRAD_CONTRACT, case["d_err32"], gs)
    print("lpips %-15s normalize %d: value err %.3g (torch fp32 %.3g, contract %.3g, bar %.3g)  grad err %.3g (torch fp32 "
          "%.3g, contract %.3g, bar %.3g)" % (shape, normalize, ve, case["v_err32"], R.OUT_CONTRACT * vs, vbar, ge,
                                              case["d_err32"], R.GRAD_CONTRACT * gs, gbar))
    assert ve <= vbar and ge <= gbar
    assert abs(float(loss.detach()) - float(values.double().mean())) <= 1e-6 * float(values.abs().max())
    assert target.grad is None and all(p.grad is None for p in net.parameters())


def test_metric_of_equal_pictures_is_exactly_zero(gpu, net):
    pkg = _pkg()
    for shape in R.METRIC_SHAPES:
        x = fill.rand(shape, 960).to(gpu)
        p = x.clone().requires_grad_(True)
        loss = pkg.ops.lpips(p, x, net)
        pkg.ops.backward(loss)
        assert float(loss.detach()) == 0.0 and float(p.grad.abs().max()) == 0.0, shape
        assert float(pkg.ops.lpips(x, x, net, reduce=False).abs().max()) == 0.0
    assert all(p.grad is None for p in net.parameters())


def test_metric_modules_and_upstream_gradients(gpu, net):
    """utils.LPIPS / utils.LPIPSLoss are ops.lpips; a backward seeded with something else than the unit seed, and the
    per-sample values under their own upstream gradients, give the matching multiples of the gradient -- each a backward
    pass of its own through the bf16x3 data-gradient kernels, whose rounding depends on the scale of what they carry, so
    the multiples agree to the gradient contract, not to the bit."""
    pkg = _pkg()
    case = R.metric_case((2, 3, 16, 16), True)
    pred, target = case["pred"].to(gpu), case["target"].to(gpu)
    values = pkg.utils.LPIPS(net)(pred, target)
    assert torch.equal(values, pkg.ops.lpips(pred, target, net, reduce=False))

    def grad_of(fn):
        p = pred.clone().requires_grad_(True)
        fn(p)
        return p.grad.detach()
    base = grad_of(lambda p: pkg.ops.backward(pkg.utils.LPIPSLoss(net)(p, target)))
    scaled = grad_of(lambda p: pkg.ops.lpips(p, target, net).backward(torch.tensor(3.0, device=gpu)))
    assert float((scaled - 3.0 * base).abs().max()) <= R.GRAD_CONTRACT * float(base.abs().max())
    per = grad_of(lambda p: pkg.ops.lpips(p, target, net, reduce=False).backward(torch.tensor([1.0, 0.0], device=gpu)))
    assert float(per[1].abs().max()) == 0.0
    assert float((per[0] - 2.0 * base[0]).abs().max()) <= R.GRAD_CONTRACT * float(base.abs().max())   # the mean halves a sample
    with pkg.ops.loss_seed(0.25, torch.full((), 0.25, device=gpu)):
        p = pred.clone().requires_grad_(True)
        loss = pkg.ops.lpips(p, target, net)
    loss.backward(torch.ones((), device=gpu))     # not the declared seed: the folded 0.25 is undone
    assert float((p.grad - base).abs().max()) <= R.GRAD_CONTRACT * float(base.abs().max())


# -- training -----------------------------------------------------------------------------------------------------------
def _oracle_step(ora, pixel, x, t, w, lr):
    """One fp32 CPU step of the oracle net on pixel + w * LPIPS (stock torch layers, torch.optim.Adam)."""
    f32, _, lins, _, _ = R.filled_net()
    opt = torch.optim.Adam(ora.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-8)
    opt.zero_grad()
    out = ora(x)
    loss = pixel(out, t) + w * R.lpips_torch(f32, lins, out, t, True).mean()
    loss.backward()
    opt.step()
    return float(loss.detach())


STEPS = {"espcn": (lambda pkg: pkg.ESPCNNet(3, 64, 2), lambda: M.ESPCN(3, 64, 2), torch.nn.functional.mse_loss, (2, 3, 16, 16)),
         "edsr": (lambda pkg: pkg.EDSRNet(3, 16, 2), lambda: M.EDSR(3, 16, 2), torch.nn.functional.l1_loss, (2, 3, 4, 4))}


@pytest.mark.parametrize("kind", sorted(STEPS))
def test_step_against_the_oracle(gpu, net, kind):
    pkg = _pkg()
    make, make_ora, pixel, in_shape = STEPS[kind]
    w, lr = 0.1, 1e-4
    ora = fill.fill_module(make_ora(), 31, 0.5 if kind == "edsr" else 1.0)
    model = make(pkg)
    model.load_state_dict(ora.state_dict())
    model.to(gpu).train()
    x, t = fill.rand(in_shape, 970), fill.rand((2, 3, 16, 16), 971)
    flat, opt, dp, step = pkg.trainers.build(kind, model, lr, lpips_weight=w, lpips_net=net)
    loss = float(step(x.to(gpu), t.to(gpu)).detach())
    want = _oracle_step(ora, pixel, x, t, w, lr)
    print("%s step with lpips_weight %.1f: loss %.9f (fp32 CPU oracle %.9f)" % (kind, w, loss, want))
    assert abs(loss - want) <= 1e-3 * abs(want)
    assert all(p.grad is None for p in net.parameters())
    got, ref = model.state_dict(), ora.state_dict()
    for n in ref:
        a, b = got[n].detach().double().cpu(), ref[n].detach().double()
        l2 = float(b.pow(2).sum().sqrt())
        assert abs(float(a.pow(2).sum().sqrt()) - l2) <= PARAM_TOL * max(l2, 1e-8), "param L2 " + n
        assert abs(float(a.sum()) - float(b.sum())) <= 10 * PARAM_TOL * max(l2, 1e-8), "param sum " + n


def test_captured_step_equals_eager(gpu, net):
    """Three ESPCN x2 steps with lpips_weight=0.1 through AutoGraph (one eager, the capture, which replays once, and a second
    replay) and three eager steps from the same parameters: the same loss bits and the same parameter bits."""
    pkg = _pkg()
    batches = [(fill.rand((2, 3, 16, 16), 975 + i).to(gpu), fill.rand((2, 3, 16, 16), 985 + i).to(gpu)) for i in range(3)]
    res = {}
    for mode in ("eager", "graph"):
        model = pkg.ESPCNNet(3, 64, 2)
        fill.fill_module(model, 5, 1.0)
        model.to(gpu).train()
        flat, opt, dp, step = pkg.trainers.build("espcn", model, 1e-2, lpips_weight=0.1, lpips_net=net)
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


def test_weight_zero_is_the_step_of_today(gpu, net, monkeypatch):
    pkg = _pkg()
    seen = []
    real = pkg.trainers.loss_segments
    monkeypatch.setattr(pkg.trainers, "loss_segments",
                        lambda model, opt, loss_fn, *a, **k: seen.append(loss_fn) or real(model, opt, loss_fn, *a, **k))
    res = []
    x, t = fill.rand((2, 3, 4, 4), 991).to(gpu), fill.rand((2, 3, 16, 16), 992).to(gpu)
    for kw in ({}, {"lpips_weight": 0.0, "lpips_net": net}, {"lpips_weight": 0.1, "lpips_net": net}):
        model = pkg.EDSRNet(3, 16, 2)
        fill.fill_module(model, 5, 1.0)
        model.to(gpu).train()
        flat, opt, dp, step = pkg.trainers.build("edsr", model, 1e-3, **kw)
        assert (seen.pop() is pkg.ops.l1_loss) == (kw.get("lpips_weight", 0.0) == 0.0)
        loss = step(x, t)
        res.append((loss.detach().clone(), flat.data.detach().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][1], res[2][1]) and float(res[2][0]) > float(res[0][0])


# -- evaluation ---------------------------------------------------------------------------------------------------------
def test_test_reports_lpips_beside_psnr(gpu, tmp_path):
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    pkg = _pkg()
    _, _, _, vgg_sd, lin_sd = R.filled_net()
    torch.save(vgg_sd, str(tmp_path / "vgg16.pth"))
    torch.save(lin_sd, str(tmp_path / "lins.pth"))
    args = cli.parse_args(["--model_name", "ESPCN", "--scale_factor", "2", "--synthetic", "--save_dir", str(tmp_path / "out"),
                           "--lpips_vgg", str(tmp_path / "vgg16.pth"), "--lpips_lin", str(tmp_path / "lins.pth")])
    t = TRAINERS["ESPCN"](args)
    t.model = fill.fill_module(t.build_model(), 7, 1.0).to(t.device).eval()
    loader = [(fill.rand((1, 3, 20, 18), 995 + i), fill.rand((1, 3, 24, 20), 997 + i)) for i in range(2)]
    psnr = t.test(loader)
    lp = t.lpips_net()
    outs = [t._infer(lr.to(gpu)) for lr, _ in loader]
    want = [float(pkg.ops.lpips(o.float(), hr.to(gpu), lp, reduce=False).mean()) for o, (_, hr) in zip(outs, loader)]
    print("test_lpips %s, per picture %s" % (t.test_lpips, want))
    assert len(psnr) == 2 and set(t.test_lpips) == {"loader"} and np.isfinite(t.test_lpips["loader"])
    assert t.test_lpips["loader"] == sum(want) / len(want) and t.test_lpips["loader"] > 0.0
    # a pair under 16 on a side stays out of the average and is no error
    small = [(fill.rand((1, 3, 14, 14), 1), fill.rand((1, 3, 12, 12), 2))] + loader
    assert len(t.test(small)) == 3 and t.test_lpips["loader"] == sum(want) / len(want)
    # without the two files nothing is reported
    t2 = TRAINERS["ESPCN"](cli.parse_args(["--model_name", "ESPCN", "--scale_factor", "2", "--synthetic", "--save_dir",
                                           str(tmp_path / "out2")]))
    t2.model = t.model
    assert t2.test(loader) == psnr and not hasattr(t2, "test_lpips")
