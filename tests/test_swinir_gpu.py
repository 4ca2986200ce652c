"""SwinIR on the GPU: the net against the fp64 plain-torch SwinIR of tests/swinir_ref.py (forward and every parameter
gradient of an L1 loss), eval's pad and crop, the train step eager against its captured graph, --resume and --ema_decay
through the common trainer, and inference: the x8 self-ensemble works, tiling is refused.

Bars: the project's standing contracts -- the forward within 1e-4, gradients within 1e-3 of fp64, relative to the
reference tensor's maximum."""
import os

import pytest
import torch

import ensemble_ref as E
import swinir_ref as R
from oracle import fill

pytestmark = pytest.mark.gpu

TOL_FWD, TOL_GRAD = 1e-4, 1e-3

SMALL = (3, 16, (2, 2), 2, 4, 2, 2, "pixelshuffle")
LIGHT = (3, 60, (2,), 6, 8, 2, 2, "pixelshuffledirect")


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _net(gpu, ctor, seed=3, gain=0.5):
    net = _pkg().SwinIRNet(*ctor)
    fill.fill_module(net, seed, gain)
    with torch.no_grad():      # LayerNorm scales around one and a bias table that matters
        for name, p in net.named_parameters():
            if "norm" in name and name.endswith("weight"):
                p.add_(1.0)
            if name.endswith("relative_position_bias_table"):
                p.mul_(20.0)
    return net.to(gpu)


@pytest.mark.parametrize("ctor,shape", [(SMALL, (2, 3, 8, 12)), (LIGHT, (1, 3, 16, 16))], ids=["dim16_ps", "dim60_direct"])
def test_net_matches_fp64_swinir(gpu, ctor, shape):
    pkg = _pkg()
    net = _net(gpu, ctor).train()
    ref = R.ref_swinir_like(net, *ctor)
    x = fill.rand(shape, 8)
    t = fill.rand((shape[0], shape[1], 2 * shape[2], 2 * shape[3]), 9)
    want = ref(x.double())
    torch.nn.functional.l1_loss(want, t.double()).backward()
    got = net(x.to(gpu))
    loss = pkg.ops.l1_loss(got, t.to(gpu))
    loss.backward()
    err = R.worst(got.detach(), want.detach())
    print("SwinIR %s forward: worst %.3e of max |ref|" % (ctor, err))
    assert err <= TOL_FWD
    wg = dict(ref.named_parameters())
    worst = ("", 0.0)
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        assert float(wg[name].grad.abs().max()) > 0.0, name
        e = R.worst(p.grad, wg[name].grad)
        worst = max(worst, (name, e), key=lambda v: v[1])
        assert e <= TOL_GRAD, (name, e)
    print("SwinIR %s gradients: worst %.3e of max |ref| (%s)" % (ctor, worst[1], worst[0]))
    net.eval()
    with torch.no_grad():       # the no-grad forward (nothing saved, inference kernels)
        assert R.worst(net(x.to(gpu)), want.detach()) <= TOL_FWD


def test_eval_pads_and_crops(gpu):
    """A 10 x 13 input is reflect-padded to 12 x 16 and the result cropped to 20 x 26; training refuses it."""
    net = _net(gpu, SMALL).eval()
    ref = R.ref_swinir_like(net, *SMALL)
    x = fill.rand((1, 3, 10, 13), 17)
    with torch.no_grad():
        got = net(x.to(gpu))
    want = ref(x.double()).detach()
    assert tuple(got.shape) == (1, 3, 20, 26)
    err = R.worst(got, want)
    print("SwinIR eval 10 x 13 (pad and crop): worst %.3e of max |ref|" % err)
    assert err <= TOL_FWD
    with pytest.raises(ValueError, match="10 x 13 input is not a multiple of the window 4"):
        net.train()(x.to(gpu))


def test_graphed_steps_equal_eager(gpu):
    """Three steps of trainers.build("swinir"): replayed from a captured graph they leave the eager run's parameters, bit
    for bit (the same kernels in the same order; no atomics in the three operators)."""
    pkg = _pkg()
    batches = [(fill.rand((2, 3, 8, 8), 50 + i).to(gpu), fill.rand((2, 3, 16, 16), 60 + i).to(gpu)) for i in range(3)]

    def make():
        net = _net(gpu, SMALL).train()
        return (net,) + tuple(pkg.trainers.build("swinir", net, 1e-3))

    net_a, flat_a, opt_a, dp_a, step_a = make()
    assert isinstance(opt_a, pkg.optim.Adam) and dp_a is None
    losses_a = [float(step_a(*b)) for b in batches]
    net_b, flat_b, opt_b, dp_b, step_b = make()
    graph = pkg.trainers.capture_step(step_b, batches[0], warmup=0, flats=[flat_b])
    losses_b = [float(graph(*b)) for b in batches]
    graph.close()
    assert losses_a == losses_b
    assert torch.equal(flat_a.data, flat_b.data)
    fresh = _net(gpu, SMALL).state_dict()      # the steps moved every parameter, tables and norms included
    for k, v in net_a.state_dict().items():
        assert not torch.equal(v, fresh[k]), k


def _args(save_dir, epochs, *extra):
    import main as cli
    return cli.parse_args(["--model_name", "SwinIR", "--swinir_dim", "16", "--swinir_depths", "2", "--swinir_heads", "2",
                           "--swinir_window", "4", "--scale_factor", "2", "--crop_size", "16", "--num_epochs", str(epochs),
                           "--batch_size", "2", "--synthetic", "--steps_per_epoch", "2", "--lr", "1e-3", "--save_dir",
                           str(save_dir), "--eager"] + list(extra))


def _run(args, seed=0):
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    torch.manual_seed(seed)
    t = TRAINERS["SwinIR"](args)
    hist = t.train()
    torch.cuda.synchronize()
    return t, hist


def test_resume_round_trip_and_ema(gpu, tmp_path):
    """1 + 1 epochs with --resume are the 2-epoch run bit for bit; --ema_decay writes a shadow with SwinIR's keys."""
    a, hist_a = _run(_args(tmp_path / "a", 2, "--save_epochs", "10", "--ema_decay", "0.9"))
    b1, hist_b1 = _run(_args(tmp_path / "b", 1, "--save_epochs", "1", "--ema_decay", "0.9"))
    assert hist_b1 == hist_a[:1]
    b2, hist_b2 = _run(_args(tmp_path / "b", 2, "--save_epochs", "10", "--ema_decay", "0.9", "--resume"), seed=123)
    assert hist_b2 == hist_a
    assert torch.equal(b2.flat.data, a.flat.data) and torch.equal(b2.optimizer.ema, a.optimizer.ema)
    assert torch.equal(b2.optimizer.exp_avg_sq, a.optimizer.exp_avg_sq)
    model_dir = os.path.join(str(tmp_path / "a"), "SwinIR", "model")
    plain = torch.load(os.path.join(model_dir, "SwinIR_param.pkl"), weights_only=True)
    ema = torch.load(os.path.join(model_dir, "SwinIR_param_ema.pkl"), weights_only=True)
    assert list(plain) == list(a.model.state_dict()) == list(ema)
    assert "layers.0.residual_group.blocks.1.attn.relative_position_bias_table" in ema
    for k in plain:
        assert plain[k].shape == ema[k].shape and not torch.equal(plain[k], ema[k]), k


def test_self_ensemble_works_and_tiling_is_refused(gpu, tmp_path):
    """test_single(img, self_ensemble=True) is ensemble_ref's composition of eight plain calls (of the fp64 net), within
    the bar of the existing ensemble tests: TOL_FWD times the largest term.  A tile is refused, naming the module."""
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    t = TRAINERS["SwinIR"](_args(tmp_path, 1))
    t.model = t.build_model()
    fill.fill_module(t.model, 5, 0.5)
    t.model.to(gpu).eval()
    ref = R.ref_swinir_like(t.model, 3, 16, (2,), 2, 4, 2, 2, "pixelshuffle")
    x = fill.rand((1, 3, 10, 14), 21)
    ys = E.terms(ref, x.double())
    want, scale = E.mean_in_order(ys), max(float(y.abs().max()) for y in ys)
    got = t.test_single(x, self_ensemble=True)
    err = float((got.double() - want).abs().max())
    print("SwinIR self-ensemble: max abs error %.3e, bar %.3e (terms up to %.3g)" % (err, TOL_FWD * scale, scale))
    assert got.shape == want.shape and err <= TOL_FWD * scale
    plain = t.test_single(x)
    assert R.worst(plain, ref(x.double()).detach()) <= TOL_FWD and not torch.equal(plain, got)
    for tile in (8, "auto"):
        with pytest.raises(ValueError, match="WindowAttention partitions the whole image into windows and cannot be tiled"):
            t.test_single(x, tile=tile)
