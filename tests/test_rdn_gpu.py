"""RDN on the GPU: the residual-dense trunk (ops.residual_dense_blocks) and the net against the fp64 plain-torch
restatement of tests/rdn_ref.py (output, input gradient and every parameter gradient), the train step eager against its
captured graph, --resume and --ema_decay through the common trainer, and inference: tiled, self-ensemble, one pass.

Bars: the project's standing contracts -- the forward within 1e-4, gradients within 1e-3 of fp64, relative to the
reference tensor's maximum, every element."""
import os

import pytest
import torch

import ensemble_ref as E
import rdn_ref as R
from conftest import rel_err
from oracle import fill

pytestmark = pytest.mark.gpu

TOL_FWD, TOL_GRAD = 1e-4, 1e-3


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


@pytest.mark.parametrize("shape", [(7, 9), (12, 10)], ids=["7x9", "12x10"])
@pytest.mark.parametrize("cfg", [(16, 16, 3, 2), (64, 32, 2, 2)], ids=["g0_16", "g0_64"])
def test_trunk_matches_fp64(gpu, cfg, shape):
    g0, g, C, D = cfg
    ops = _pkg().ops
    blocks = R.make_blocks(g0, g, C, D, 40 + g0)
    x = R.rand((2, g0) + shape, 3)
    gy = R.rand((2, D * g0) + shape, 4)
    x64 = x.double().requires_grad_(True)
    b64 = [tuple(p.double().requires_grad_(True) for p in b) for b in blocks]
    want = R.trunk_forward(x64, b64)
    want.backward(gy.double())
    xd = x.to(gpu).requires_grad_(True)
    bd = [tuple(p.to(gpu).requires_grad_(True) for p in b) for b in blocks]
    got = ops.residual_dense_blocks(xd, bd)
    assert tuple(got.shape) == (2, D * g0) + shape and got.is_contiguous(memory_format=torch.channels_last)
    got.backward(gy.to(gpu))
    err = R.worst(got.detach(), want.detach())
    print("trunk %s %s forward: worst %.3e of max |ref|" % (cfg, shape, err))
    assert err <= TOL_FWD
    # the returned tensor is the fusion buffer: block d's output is channel slice d
    h = x.double()
    for d in range(D):
        h = R.rdb_forward(h, [p.detach() for p in b64[d]])
        assert R.worst(got.detach()[:, d * g0:(d + 1) * g0], h) <= TOL_FWD, d
    e = R.worst(xd.grad, x64.grad)
    worst = ("dx", e)
    assert e <= TOL_GRAD
    for d in range(D):
        for i, (p, q) in enumerate(zip(bd[d], b64[d])):
            assert p.grad is not None and p.grad.shape == p.shape, (d, i)
            e = R.worst(p.grad, q.grad)
            worst = max(worst, ("block %d param %d" % (d, i), e), key=lambda v: v[1])
            assert e <= TOL_GRAD, (d, i, e)
    print("trunk %s %s gradients: worst %.3e of max |ref| (%s)" % (cfg, shape, worst[1], worst[0]))
    # two calls, the same bits; and the no-grad forward on parameters that require grad (the inference path: see the
    # growth-buffer test below)
    xd2 = x.to(gpu).requires_grad_(True)
    bd2 = [tuple(p.detach().clone().requires_grad_(True) for p in b) for b in bd]
    got2 = ops.residual_dense_blocks(xd2, bd2)
    got2.backward(gy.to(gpu))
    assert torch.equal(got2, got) and torch.equal(xd2.grad, xd.grad)
    assert all(torch.equal(p.grad, q.grad) for b, c in zip(bd, bd2) for p, q in zip(b, c))
    with torch.no_grad():
        assert R.worst(ops.residual_dense_blocks(x.to(gpu), bd), want.detach()) <= TOL_FWD


@pytest.mark.parametrize("how", ["no_grad_on_trainable_parameters", "nothing_requires_grad"])
def test_a_forward_without_a_backward_keeps_one_growth_buffer(gpu, how, monkeypatch):
    """test(), test_single, --tile and --self_ensemble run the TRAINING model under torch.no_grad(): its parameters require
    grad, and the op must still take the inference path -- one growth buffer shared by all D blocks (what
    tiling.net_geometry's floats_per_pixel counts), nothing saved, no graph.  With a backward ahead it keeps one a block."""
    ops = _pkg().ops
    g0, g, C, D = 16, 16, 2, 3
    made = []
    real = ops._growth_buffer
    monkeypatch.setattr(ops, "_growth_buffer", lambda *a: made.append(a[1]) or real(*a))
    trainable = how == "no_grad_on_trainable_parameters"
    blocks = [tuple(p.to(gpu).requires_grad_(trainable) for p in b) for b in R.make_blocks(g0, g, C, D, 7)]
    x = R.rand((2, g0, 7, 9), 3).to(gpu).contiguous(memory_format=torch.channels_last)   # (no layout copy inside)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        out = ops.residual_dense_blocks(x, blocks)
    peak = torch.cuda.max_memory_allocated() - before
    assert made == [C * g] and out.grad_fn is None and not out.requires_grad
    pixels = 2 * 7 * 9
    assert peak <= 4 * pixels * (D * g0 + C * g) + 4096          # the fusion buffer and ONE growth buffer (+ rounding)
    with torch.no_grad():
        assert torch.equal(out, ops.residual_dense_blocks(x, [tuple(p.detach() for p in b) for b in blocks]))
    if trainable:
        del made[:]
        kept = ops.residual_dense_blocks(x, blocks)
        assert made == [C * g] * D and kept.grad_fn is not None and torch.equal(kept, out)


def _net(gpu, ctor, seed=3, gain=0.7):
    net = _pkg().RDNNet(*ctor)
    fill.fill_module(net, seed, gain)
    return net.to(gpu)


@pytest.mark.parametrize("scale", (2, 3, 4))
def test_net_matches_fp64_rdn(gpu, scale):
    pkg = _pkg()
    ctor = (3, 16, 2, 3, 16, scale)
    shape = (2, 3, 7, 9) if scale == 3 else (2, 3, 12, 10)
    net = _net(gpu, ctor).train()
    ref = R.ref_rdn_like(net, *ctor)
    x = fill.rand(shape, 8)
    t = fill.rand((shape[0], shape[1], scale * shape[2], scale * shape[3]), 9)
    want = ref(x.double())
    torch.nn.functional.l1_loss(want, t.double()).backward()
    got = net(x.to(gpu))
    loss = pkg.ops.l1_loss(got, t.to(gpu))
    loss.backward()
    err = R.worst(got.detach(), want.detach())
    print("RDN %s forward: worst %.3e of max |ref|" % (ctor, err))
    assert got.shape == want.shape and err <= TOL_FWD
    wg = dict(ref.named_parameters())
    worst = ("", 0.0)
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        e = R.worst(p.grad, wg[name].grad)
        worst = max(worst, (name, e), key=lambda v: v[1])
        assert e <= TOL_GRAD, (name, e)
    print("RDN %s gradients: worst %.3e of max |ref| (%s)" % (ctor, worst[1], worst[0]))
    net.eval()
    with torch.no_grad():       # the no-grad forward (nothing saved, inference kernels)
        assert R.worst(net(x.to(gpu)), want.detach()) <= TOL_FWD


def test_graphed_steps_equal_eager(gpu):
    """Three steps of trainers.build("rdn"): replayed from a captured graph they leave the eager run's parameters, bit for
    bit (the same kernels in the same order, every buffer from torch's allocator, no atomics in the slice convolutions)."""
    pkg = _pkg()
    ctor = (3, 32, 2, 2, 16, 2)
    batches = [(fill.rand((4, 3, 8, 8), 50 + i).to(gpu), fill.rand((4, 3, 16, 16), 60 + i).to(gpu)) for i in range(3)]

    def make():
        net = _net(gpu, ctor).train()
        return (net,) + tuple(pkg.trainers.build("rdn", net, 1e-3))

    net_a, flat_a, opt_a, dp_a, step_a = make()
    assert isinstance(opt_a, pkg.optim.Adam) and dp_a is None
    losses_a = [float(step_a(*b)) for b in batches]
    net_b, flat_b, opt_b, dp_b, step_b = make()
    graph = pkg.trainers.capture_step(step_b, batches[0], warmup=0, flats=[flat_b])
    losses_b = [float(graph(*b)) for b in batches]
    graph.close()
    assert losses_a == losses_b
    assert torch.equal(flat_a.data, flat_b.data)
    fresh = _net(gpu, ctor).state_dict()      # the steps moved every parameter, the blocks' included
    for k, v in net_a.state_dict().items():
        assert not torch.equal(v, fresh[k]), k


def _args(save_dir, epochs, *extra):
    import main as cli
    return cli.parse_args(["--model_name", "RDN", "--rdn_blocks", "2", "--rdn_layers", "2", "--rdn_growth", "16",
                           "--scale_factor", "2", "--crop_size", "16", "--num_epochs", str(epochs), "--batch_size", "2",
                           "--synthetic", "--steps_per_epoch", "2", "--lr", "1e-3", "--save_dir", str(save_dir), "--eager"]
                          + list(extra))


def _run(args, seed=0):
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    torch.manual_seed(seed)
    t = TRAINERS["RDN"](args)
    hist = t.train()
    torch.cuda.synchronize()
    return t, hist


def test_resume_round_trip_and_ema(gpu, tmp_path):
    """1 + 1 epochs with --resume are the 2-epoch run bit for bit; --ema_decay writes a shadow with RDN's keys."""
    a, hist_a = _run(_args(tmp_path / "a", 2, "--save_epochs", "10", "--ema_decay", "0.9"))
    b1, hist_b1 = _run(_args(tmp_path / "b", 1, "--save_epochs", "1", "--ema_decay", "0.9"))
    assert hist_b1 == hist_a[:1]
    b2, hist_b2 = _run(_args(tmp_path / "b", 2, "--save_epochs", "10", "--ema_decay", "0.9", "--resume"), seed=123)
    assert hist_b2 == hist_a
    assert torch.equal(b2.flat.data, a.flat.data) and torch.equal(b2.optimizer.ema, a.optimizer.ema)
    assert torch.equal(b2.optimizer.exp_avg_sq, a.optimizer.exp_avg_sq)
    model_dir = os.path.join(str(tmp_path / "a"), "RDN", "model")
    plain = torch.load(os.path.join(model_dir, "RDN_param.pkl"), weights_only=True)
    ema = torch.load(os.path.join(model_dir, "RDN_param_ema.pkl"), weights_only=True)
    assert list(plain) == list(a.model.state_dict()) == list(ema)
    assert "RDBs.1.convs.1.conv.0.weight" in ema and "RDBs.0.LFF.bias" in ema
    for k in plain:
        assert plain[k].shape == ema[k].shape and not torch.equal(plain[k], ema[k]), k


def _inference_trainer(gpu, tmp_path):
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    t = TRAINERS["RDN"](_args(tmp_path, 1))
    t.model = t.build_model()
    fill.fill_module(t.model, 5, 0.7)
    t.model.to(gpu).eval()
    return t, R.ref_rdn_like(t.model, 3, 64, 2, 2, 16, 2).eval()


def test_single_tiled(gpu, tmp_path):
    """test_single(img, tile=...) against the fp64 net's ONE-PASS output, under the contract of tests/test_tile_gpu.py: at
    least 2 x 3 tiles with the last row and column shifted inwards, every chunking within the forward bar."""
    from pytorch_super_resolution_model_collection_amd import tiling
    t, ref = _inference_trainer(gpu, tmp_path)
    tile = 26
    x = fill.rand((1, 3, 45, 67), 31)
    plan = tiling.plan(tiling.net_geometry(t.model), 45, 67, tile)
    assert len(plan.rows) >= 2 and len(plan.cols) >= 3
    assert plan.rows.starts[-1] == plan.H - plan.th and plan.cols.starts[-1] == plan.W - plan.tw   # shifted inwards
    assert (plan.H - plan.th) % plan.rows.starts[1] and (plan.W - plan.tw) % plan.cols.starts[1]
    with torch.no_grad():
        want = ref(x.double())
    got = t.test_single(x, tile=tile)
    assert torch.is_tensor(got) and not got.is_cuda and got.shape == want.shape
    err = rel_err(got, want)
    print("RDN tile=%d (%d x %d tiles): tiled vs fp64 one pass rel_err %.3e" % (tile, len(plan.rows), len(plan.cols), err))
    assert err < TOL_FWD
    for tb in (1, "all"):
        assert rel_err(t.test_single(x[0], tile=tile, tile_batch=tb), want) < TOL_FWD, tb
    one_pass = t.test_single(x)
    assert rel_err(one_pass, want) < TOL_FWD
    assert torch.equal(t.test_single(x, tile="auto"), one_pass)       # this small picture stays in one pass
    t.args.tile = tile                                                 # the option of the command line
    assert torch.equal(t.test_single(x), got)


def test_self_ensemble_and_test_single(gpu, tmp_path):
    """test_single(img, self_ensemble=True) is ensemble_ref's composition of eight plain calls (of the fp64 net), within
    the bar of the existing ensemble tests: TOL_FWD times the largest term."""
    t, ref = _inference_trainer(gpu, tmp_path)
    x = fill.rand((1, 3, 10, 14), 21)
    ys = E.terms(ref, x.double())
    want, scale = E.mean_in_order(ys), max(float(y.abs().max()) for y in ys)
    got = t.test_single(x, self_ensemble=True)
    err = float((got.double() - want).abs().max())
    print("RDN self-ensemble: max abs error %.3e, bar %.3e (terms up to %.3g)" % (err, TOL_FWD * scale, scale))
    assert got.shape == want.shape and err <= TOL_FWD * scale
    plain = t.test_single(x)
    with torch.no_grad():
        assert R.worst(plain, ref(x.double())) <= TOL_FWD and not torch.equal(plain, got)
