"""Train-trajectory parity on the MI355X: the reference's train-step bodies (transcribed in the
oracle and pinned bit-for-bit against the reference when the fixtures were generated) vs the HIP
path, 3 steps each: losses + parameter fingerprints (full final parameters for config c1)."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import fill

pytestmark = pytest.mark.gpu
TOL = 2e-4  # contract 1e-3


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _check_params(net, golden, tag, tol=TOL):
    names = [str(n) for n in golden[tag + ".param_names"]]
    sums = golden[tag + ".param_sums"]
    sd = net.state_dict()
    for n, (s, l2) in zip(names, sums):
        t = sd[n].detach().double().cpu()
        assert abs(float(t.pow(2).sum().sqrt()) - l2) <= tol * max(l2, 1e-8), "param L2 " + n
        assert abs(float(t.sum()) - s) <= 10 * tol * max(l2, 1e-8), "param sum " + n


def _run(gpu, kind, net, lr, batches, gain):
    pkg = _pkg()
    fill.fill_module(net, 99, gain)
    net.to(gpu).train()
    flat, opt, dp, step = pkg.trainers.build(kind, net, lr)
    losses = []
    for b in batches:
        out = step(*[t.to(gpu) for t in b])
        outs = out if isinstance(out, tuple) else (out,)
        losses.append(sum(float(o) for o in outs))
    return losses


B = fill.rand


@pytest.mark.parametrize("lr,tag", [(1e-5, "srcnn_c1_lr1e-5"), (1e-2, "srcnn_c1_lr1e-2")])
def test_srcnn_c1(gpu, train_golden, lr, tag):
    """BASELINE config c1 exactly: SRCNN x2, B=16, 3x64x64 -> 3x48x48, MSE, SGD."""
    pkg = _pkg()
    net = pkg.SRCNNNet(3, 64)
    batches = [(B((16, 3, 64, 64), 10 + i), B((16, 3, 48, 48), 20 + i)) for i in range(3)]
    losses = _run(gpu, "srcnn", net, lr, batches, 1.0)
    assert rel_err(np.array(losses), train_golden[tag + ".losses"]) < TOL
    _check_params(net, train_golden, tag)
    if lr == 1e-2:
        for k, v in net.state_dict().items():
            assert rel_err(v, train_golden["%s.final.%s" % (tag, k)]) < TOL, k


def test_fsrcnn(gpu, train_golden):
    pkg = _pkg()
    net = pkg.FSRCNNNet(3, 4, 56, 12, 4)
    batches = [(B((4, 3, 12, 12), 30 + i), B((4, 3, 32, 32), 40 + i)) for i in range(3)]
    losses = _run(gpu, "fsrcnn", net, 1e-3, batches, 1.0)
    assert rel_err(np.array(losses), train_golden["fsrcnn.losses"]) < TOL
    _check_params(net, train_golden, "fsrcnn")


def test_vdsr_with_clip(gpu, train_golden):
    pkg = _pkg()
    net = pkg.VDSRNet(3, 64, 18)
    batches = [(B((4, 3, 17, 17), 50 + i), B((4, 3, 17, 17), 60 + i)) for i in range(3)]
    losses = _run(gpu, "vdsr", net, 1e-2, batches, 1.0)
    assert rel_err(np.array(losses), train_golden["vdsr.losses"]) < TOL
    _check_params(net, train_golden, "vdsr")


def test_edsr_l1_adam(gpu, train_golden):
    pkg = _pkg()
    net = pkg.EDSRNet(3, 64, 16)
    batches = [(B((4, 3, 8, 8), 70 + i), B((4, 3, 32, 32), 80 + i)) for i in range(3)]
    losses = _run(gpu, "edsr", net, 1e-4, batches, 0.5)
    assert rel_err(np.array(losses), train_golden["edsr.losses"]) < TOL
    _check_params(net, train_golden, "edsr")


def test_lapsrn_shared_weights(gpu, train_golden):
    pkg = _pkg()
    net = pkg.LapSRNNet(3, 64, 10)
    batches = [(B((2, 3, 8, 8), 90 + i), B((2, 3, 16, 16), 100 + i), B((2, 3, 32, 32), 110 + i)) for i in range(3)]
    losses = _run(gpu, "lapsrn", net, 1e-4, batches, 1.0)
    assert rel_err(np.array(losses), train_golden["lapsrn.losses"]) < TOL
    _check_params(net, train_golden, "lapsrn")


def test_srgan_adversarial_step(gpu, train_golden):
    pkg = _pkg()
    G, D = pkg.SRGANGenerator(3, 64, 16), pkg.SRGANDiscriminator(3, 64, 32)
    fill.fill_module(G, 5, 0.7)
    fill.fill_module(D, 6, 1.0)
    G.to(gpu).train()
    D.to(gpu).train()
    g_opt = pkg.optim.make_optimizer("srgan_g", pkg.optim.FlatParams(G), 1e-4)
    d_opt = pkg.optim.make_optimizer("srgan_d", pkg.optim.FlatParams(D), 1e-2)
    step = pkg.trainers.srgan_step(G, D, g_opt, d_opt)
    losses = []
    for i in range(2):
        d_loss, g_loss = step(B((4, 3, 8, 8), 120 + i).to(gpu), B((4, 3, 32, 32), 130 + i).to(gpu))
        losses.append((float(d_loss), float(g_loss)))
    assert rel_err(np.array(losses), train_golden["srgan.losses"]) < 5e-4
    _check_params(G, train_golden, "srgan.G", 5e-4)
    _check_params(D, train_golden, "srgan.D", 5e-4)


@pytest.mark.parametrize("forced", [False, True], ids=["default_kernels", "wave_specialised_kernels"])
def test_graphed_step_equals_eager(gpu, monkeypatch, forced):
    """hipGraph-captured step (zero_grad+fwd+loss+bwd+clip+SGD) reproduces the eager trajectory.  forced: the kernels a
    benchmark-size VDSR step runs (k_conv_bfw channel slices forward and backward, pre-masked gradients, the persistent
    first-layer kernel) on this small problem -- the marks that let a layer skip its masks are decided at capture time."""
    pkg = _pkg()
    if forced:
        monkeypatch.setenv("SRK_BFW", "1")
        monkeypatch.setenv("SRK_ROWSW", "1")
        monkeypatch.setenv("SRK_BF3_DIRECT", "0")
        monkeypatch.setattr(pkg.ops, "F16X3_ALWAYS", True)
        pkg.ops.PREMASK_STATS.update(masked_dx=0, masks_skipped=0)
    batches = [(B((4, 3, 17, 17), 50 + i).to(gpu), B((4, 3, 17, 17), 60 + i).to(gpu)) for i in range(4)]

    def make():
        net = pkg.VDSRNet(3, 64, 4)
        fill.fill_module(net, 3, 1.0)
        net.to(gpu).train()
        flat = pkg.optim.FlatParams(net)
        return net, pkg.optim.make_optimizer("vdsr", flat, 1e-2)

    net_a, opt_a = make()
    step = pkg.trainers.mse_step(net_a, opt_a, None, clip=0.4)
    ref_losses = [float(step(*b)) for b in batches]
    net_b, opt_b = make()
    snapshot = opt_b.flat.data.clone()
    g = pkg.trainers.GraphedStep(net_b, opt_b, pkg.ops.mse_loss, batches[0], clip=0.4, warmup=2)
    # warm-up steps moved the parameters: restore the initial state before the measured replay
    opt_b.flat.data.copy_(snapshot)
    opt_b.buf.zero_()
    losses = [float(g(*b)) for b in batches]
    assert rel_err(np.array(losses), np.array(ref_losses)) < 1e-5
    assert rel_err(opt_b.flat.data, opt_a.flat.data) < 1e-5
    if forced:
        assert pkg.ops.PREMASK_STATS["masked_dx"] > 0 and pkg.ops.PREMASK_STATS["masks_skipped"] > 0


@pytest.mark.parametrize("model", ["edsr", "fsrcnn", "espcn", "srcnn", "lapsrn", "srgan_g", "srgan_d", "srgan_d_small"])
def test_pack_plan_equals_per_layer_pack(gpu, model):
    """One srk_pack_weights_batched launch writes byte-for-byte what the per-layer pack calls write
    (fp32 + bf16x3 layouts, forward + data-gradient, pixel-shuffle filter/bias order, deconv)."""
    pkg = _pkg()
    net = {"edsr": lambda: pkg.EDSRNet(3, 64, 4), "fsrcnn": lambda: pkg.FSRCNNNet(1, 3, 56, 12, 4),
           "espcn": lambda: pkg.ESPCNNet(3, 64, 4), "srcnn": lambda: pkg.SRCNNNet(3, 64), "lapsrn": lambda: pkg.LapSRNNet(1, 64, 4),
           "srgan_g": lambda: pkg.SRGANGenerator(3, 64, 2),
           # 64 .. 512-channel filters (the LDS-tiled fast path) / 8 .. 64 channels (padded layouts: the generic path)
           "srgan_d": lambda: pkg.SRGANDiscriminator(3, 64, 32),
           "srgan_d_small": lambda: pkg.SRGANDiscriminator(3, 8, 32)}[model]()
    fill.fill_module(net, 11, 1.0)
    net.to(gpu)
    from pytorch_super_resolution_model_collection_amd._lib import check, load, ptr, stream_ptr
    lib = load()
    flat = pkg.optim.FlatParams(net)
    plan = flat.plan
    assert plan.n > 0 and not plan.current()
    plan.buf.zero_()
    plan.pack()
    torch.cuda.synchronize()
    assert plan.current()
    for m, fo, nf, bo, nb, bp_off, cout, ps_r in plan.layers:
        tr = isinstance(m, pkg.layers.ConvTranspose2d)
        cin, kh, kw = m.weight.shape[0 if tr else 1], m.weight.shape[2], m.weight.shape[3]
        _, _, wpf, bp, wpb, _, _ = m._plan
        # per-layer packs into zeroed buffers (the layouts have alignment gaps no kernel writes)
        ref_f, ref_b = torch.zeros_like(wpf), torch.zeros_like(wpb)
        w = m.weight.detach()
        check(lib.srk_pack_weight_fwd(ptr(w), ptr(ref_f), cout, cin, kh, kw, int(tr), ps_r, stream_ptr()), "fwd")
        check(lib.srk_pack_weight_bwd(ptr(w), ptr(ref_b), cout, cin, kh, kw, int(tr), ps_r, stream_ptr()), "bwd")
        assert torch.equal(wpf.view(torch.int32), ref_f.view(torch.int32)), (model, tuple(m.weight.shape), "fwd")
        assert torch.equal(wpb.view(torch.int32), ref_b.view(torch.int32)), (model, tuple(m.weight.shape), "bwd")
        if bp is not None:
            assert torch.equal(bp, pkg.ops.pack_bias_ps(m.bias.detach(), ps_r))
        views = pkg.layers._plan_views(m, ps_r)
        assert views is not None and views[0].data_ptr() == wpf.data_ptr()
    # a host-side edit of one parameter invalidates just that layer's views; an optimizer step all of them
    first = plan.layers[0][0]
    with torch.no_grad():
        first.weight.mul_(1.0)
    assert pkg.layers._plan_views(first, plan.layers[0][7]) is None
    flat.epoch += 1
    assert not plan.current()


def test_flat_params_keep_state_dict_and_grads(gpu):
    pkg = _pkg()
    net = pkg.ESPCNNet(3, 64, 4)
    fill.fill_module(net, 1)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net.to(gpu)
    flat = pkg.optim.FlatParams(net)
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), before[k])
    for p in net.parameters():
        assert p.grad is not None and p.grad.data_ptr() == p._srk_grad.data_ptr()
        assert p.data_ptr() % 16 == 0
    assert flat.numel >= sum(p.numel() for p in net.parameters())


def test_trainer_objects_and_cli(gpu, tmp_path):
    """The reference's trainer surface: MODEL(args).train()/test()/save_model()/load_model() driven by
    main.py's flags, on synthetic patches; checkpoints reload into the CPU oracle (same state_dict)."""
    import main as cli
    from oracle import ref_modules as R
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    for name, extra in (("EDSR", ["--crop_size", "32"]), ("VDSR", ["--crop_size", "17"]),
                        ("ESPCN", ["--crop_size", "48"]), ("SRGAN", ["--crop_size", "32", "--batch_size", "2", "--epoch_pretrain", "1"])):
        args = cli.parse_args(["--model_name", name, "--num_epochs", "2", "--save_epochs", "1", "--batch_size", "2",
                               "--synthetic", "--steps_per_epoch", "2", "--lr", "1e-4", "--save_dir", str(tmp_path)] + extra)
        t = TRAINERS[name](args)
        hist = t.train()
        assert len(hist) == 2
        assert all(np.isfinite(np.array(hist)).ravel())
        assert t.load_model()
        psnr = t.test()
        assert isinstance(psnr, list)
    # EDSR checkpoint written with the reference's file-name pattern loads into the oracle
    import glob
    files = glob.glob(str(tmp_path / "EDSR" / "model" / "EDSR_param_ch3_batch2_epoch2_lr0.0001.pkl"))
    assert files, "EDSR checkpoint name does not follow edsr.py:329-335"
    R.EDSR(3, 64, 16).load_state_dict(torch.load(files[0]))


def test_trainer_refuses_a_missing_training_folder(gpu, tmp_path):
    """Without --synthetic a mistyped --data_dir / --train_dataset is an error (the reference crashes in its DataLoader);
    round-2 advisor finding: the trainer used to fall back to random patches silently."""
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    for name in ("EDSR", "SRGAN"):
        args = cli.parse_args(["--model_name", name, "--num_epochs", "1", "--batch_size", "2", "--crop_size", "32",
                               "--data_dir", str(tmp_path / "nowhere"), "--train_dataset", "DIV2K",
                               "--save_dir", str(tmp_path / "out")])
        with pytest.raises(FileNotFoundError, match="--synthetic"):
            TRAINERS[name](args).train()


def test_trainer_replays_its_step_as_a_graph(gpu, tmp_path):
    """MODEL(args).train() captures its step after the first batch of a shape and replays it (sr_trainers._Trainer._step);
    --eager launches every kernel from Python.  Same data, same seeds: the same loss history and the same checkpoint,
    across a learning-rate decay (a device scalar the captured optimizer kernel reads) and for SGD + clipping (VDSR) as well as Adam (EDSR)."""
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS, LR_DECAY
    pkg = _pkg()
    for name, extra, epochs in (("EDSR", ["--crop_size", "32"], 3), ("VDSR", ["--crop_size", "17"], 3),
                                ("LapSRN", ["--crop_size", "32"], 3)):
        hist, params = {}, {}
        old = dict(LR_DECAY)
        LR_DECAY[name.lower()] = (2, 2.0)        # decay after the 2nd epoch: the replayed graph must pick the new rate up
        try:
            for mode in ("graph", "eager"):
                args = cli.parse_args(["--model_name", name, "--num_epochs", str(epochs), "--save_epochs", "10",
                                       "--batch_size", "2", "--synthetic", "--steps_per_epoch", "4", "--lr", "1e-3",
                                       "--save_dir", str(tmp_path / mode)] + extra + (["--eager"] if mode == "eager" else []))
                torch.manual_seed(0)
                t = TRAINERS[name](args)
                hist[mode] = t.train()
                params[mode] = t.flat.data.detach().clone()
                if mode == "graph":
                    assert t._graph is None     # closed at the end of train()
        finally:
            LR_DECAY.clear()
            LR_DECAY.update(old)
        for a, b in zip(hist["graph"], hist["eager"]):
            assert abs(a - b) <= 2e-5 * abs(b) + 1e-9, (name, hist)
        assert rel_err(params["graph"], params["eager"]) < (5e-3 if name in ("EDSR", "LapSRN") else 1e-5), name   # Adam: +-lr sign flips
    # SRGAN: generator pre-training (GraphedStep) and the two-model adversarial step (GraphedFn) replayed as graphs
    hist = {}
    for mode in ("graph", "eager"):
        args = cli.parse_args(["--model_name", "SRGAN", "--num_epochs", "2", "--save_epochs", "10", "--batch_size", "2",
                               "--synthetic", "--steps_per_epoch", "4", "--lr", "1e-4", "--crop_size", "32", "--epoch_pretrain", "1",
                               "--save_dir", str(tmp_path / ("gan_" + mode))] + (["--eager"] if mode == "eager" else []))
        torch.manual_seed(0)
        hist[mode] = TRAINERS["SRGAN"](args).train()
    for (d0, g0), (d1, g1) in zip(hist["graph"], hist["eager"]):
        assert abs(d0 - d1) <= 1e-3 * abs(d1) + 1e-6 and abs(g0 - g1) <= 1e-3 * abs(g1) + 1e-6, hist


def test_fused_skip_gradient_matches_axpby_fan_in(gpu):
    """ops.GradBox (the residual blocks' skip gradient added by conv1's data-gradient epilogue) against the unfused
    fan-in (ops.fork + srk_axpby): same parameter gradients up to summation order, also when backward runs twice over
    a retained graph (the box is refilled by every backward pass) and when the block input needs no gradient."""
    pkg = _pkg()
    x, t = B((4, 3, 12, 12), 81).to(gpu), B((4, 3, 48, 48), 82).to(gpu)
    grads = []
    for fused in (False, True):
        pkg.ops.FUSE_SKIP_GRAD = fused
        try:
            net = pkg.EDSRNet(3, 64, 4)
            fill.fill_module(net, 3, 0.5)
            net.to(gpu).train()
            flat = pkg.optim.FlatParams(net)
            flat.zero_grad()
            loss = pkg.ops.l1_loss(net(x), t)
            loss.backward(retain_graph=True)
            g1 = flat.grad.clone()
            loss.backward()  # accumulates a second, identical contribution
            grads.append((g1, flat.grad.clone()))
        finally:
            pkg.ops.FUSE_SKIP_GRAD = True
    (a1, a2), (b1, b2) = grads
    assert float(a1.abs().max()) > 0
    assert rel_err(b1, a1) < 1e-5
    assert rel_err(a2, 2 * a1) < 1e-5 and rel_err(b2, 2 * b1) < 1e-5
    # a residual block fed by a tensor that needs no gradient: no box, no fan-in, weights still get gradients
    blk = pkg.base_networks.ResnetBlock(64, norm=None)
    fill.fill_module(blk, 5, 0.5)
    blk.to(gpu).train()
    xin = B((2, 64, 9, 9), 83).to(gpu)
    blk(xin).sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in blk.parameters())


def test_graphed_srgan_step_equals_eager(gpu):
    """trainers.GraphedFn around the SRGAN adversarial step (two models, two optimizers, BatchNorm running statistics,
    weight re-packing after each optimizer step all inside one hipGraph): same loss trajectory as the eager step."""
    pkg = _pkg()
    batches = [(B((4, 3, 8, 8), 90 + i).to(gpu), B((4, 3, 32, 32), 95 + i).to(gpu)) for i in range(3)]

    def make():
        G, D = pkg.SRGANGenerator(3, 16, 2), pkg.SRGANDiscriminator(3, 8, 32)
        fill.fill_module(G, 5, 0.7)
        fill.fill_module(D, 6, 1.0)
        G.to(gpu).train()
        D.to(gpu).train()
        g_opt = pkg.optim.make_optimizer("srgan_g", pkg.optim.FlatParams(G), 1e-4)
        d_opt = pkg.optim.make_optimizer("srgan_d", pkg.optim.FlatParams(D), 1e-2)
        return G, D, g_opt, d_opt, pkg.trainers.srgan_step(G, D, g_opt, d_opt)

    Ga, Da, ga, da, step_a = make()
    ref = [[float(v) for v in step_a(*b)] for b in batches]
    Gb, Db, gb, db, step_b = make()
    def state(o):
        return [o.flat.data] + [getattr(o, k) for k in ("buf", "exp_avg", "exp_avg_sq", "step_dev")
                                if getattr(o, k, None) is not None]

    snap = [[t.clone() for t in state(o)] for o in (gb, db)]
    bn_state = [(m, m.running_mean.clone(), m.running_var.clone()) for net in (Gb, Db) for m in net.modules()
                if isinstance(m, torch.nn.BatchNorm2d) and m.running_mean is not None]
    graphed = pkg.trainers.GraphedFn(step_b, batches[0], warmup=2)
    # the warm-up / capture calls moved the state: restore it before the measured replays
    for o, saved in zip((gb, db), snap):
        for t, t0 in zip(state(o), saved):
            t.copy_(t0)
    for m, rm, rv in bn_state:
        m.running_mean.copy_(rm)
        m.running_var.copy_(rv)
    got = [[float(v) for v in graphed(*b)] for b in batches]
    assert rel_err(np.array(got), np.array(ref)) < 1e-4



def test_graphed_steps_interleaved_with_eval_forwards(gpu):
    """A hipGraph replay runs the optimizer kernel without optim.step()'s host bookkeeping; no-grad forwards cache
    their packed filters (layers._PackCache).  train(graph) -> eval -> train(graph) -> eval must see the NEW weights in
    the second eval: compare each eval output with a fresh model that loads the current state_dict."""
    pkg = _pkg()
    x, t = B((4, 3, 12, 12), 31).to(gpu), B((4, 3, 48, 48), 32).to(gpu)
    probe = B((2, 3, 10, 10), 33).to(gpu)
    net = pkg.EDSRNet(3, 64, 2)
    fill.fill_module(net, 3, 0.5)
    net.to(gpu).train()
    flat, opt, dp, step = pkg.trainers.build("edsr", net, 1e-2)
    graphed = pkg.trainers.GraphedStep(net, opt, pkg.ops.l1_loss, (x, t), warmup=1)
    outs = []
    for _ in range(3):
        graphed(x, t)
        net.eval()
        with torch.no_grad():
            y = net(probe).clone()
        net.train()
        fresh = pkg.EDSRNet(3, 64, 2)
        fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
        fresh.to(gpu).eval()
        with torch.no_grad():
            want = fresh(probe)
        assert torch.equal(y, want), "eval forward after a graph replay used stale packed filters"
        outs.append(y)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])  # lr 1e-2: the weights do move

    # GraphedFn: same property through the generic wrapper
    net2 = pkg.EDSRNet(3, 64, 2)
    fill.fill_module(net2, 3, 0.5)
    net2.to(gpu).train()
    flat2, opt2, _, step2 = pkg.trainers.build("edsr", net2, 1e-2)
    gfn = pkg.trainers.GraphedFn(step2, (x, t), warmup=1, flats=[flat2])
    prev = None
    for _ in range(2):
        gfn(x, t)
        net2.eval()
        with torch.no_grad():
            y = net2(probe).clone()
        net2.train()
        fresh = pkg.EDSRNet(3, 64, 2)
        fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in net2.state_dict().items()})
        fresh.to(gpu).eval()
        with torch.no_grad():
            assert torch.equal(y, fresh(probe))
        assert prev is None or not torch.equal(prev, y)
        prev = y


def test_graphed_two_model_step_repacks_what_others_changed(gpu):
    """The captured SRGAN step packs a model's filters only where its own updates made them stale (the discriminator is
    NOT re-packed at the start of a step).  Parameters changed from outside between two replays -- here: D scaled in
    place, as a load_state_dict or a broadcast would -- must still reach the next replay (trainers._repack_touched)."""
    pkg = _pkg()
    res = {}
    for mode in ("graph", "eager"):
        G, D = pkg.SRGANGenerator(3, 64, 2), pkg.SRGANDiscriminator(3, 64, 32)
        fill.fill_module(G, 11, 0.5)
        fill.fill_module(D, 12, 0.5)
        G.to(gpu).train()
        D.to(gpu).train()
        gflat, dflat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
        g_opt = pkg.optim.make_optimizer("srgan_g", gflat, 1e-4)
        d_opt = pkg.optim.make_optimizer("srgan_d", dflat, 1e-4)
        lr, hr = B((4, 3, 8, 8), 81).to(gpu), B((4, 3, 32, 32), 82).to(gpu)
        step = pkg.trainers.srgan_step(G, D, g_opt, d_opt, lazy_pack=True)
        if mode == "graph":
            step = pkg.trainers.GraphedFn(step, (lr, hr), warmup=1, flats=[gflat, dflat])
        else:
            step(lr, hr)                      # the graph's warm-up call
        losses = []
        for i in range(4):
            if i == 2:                        # somebody else rewrites D between two steps
                dflat.data.mul_(0.5)
                dflat.mark_changed()
            d, g = step(lr, hr)
            losses.append((float(d), float(g)))
        res[mode] = losses
    for (d0, g0), (d1, g1) in zip(res["graph"], res["eager"]):
        assert abs(d0 - d1) <= 1e-3 * abs(d1) + 1e-6 and abs(g0 - g1) <= 1e-3 * abs(g1) + 1e-6, res
    assert abs(res["eager"][2][0] - res["eager"][1][0]) > 1e-3 * abs(res["eager"][1][0])   # the rewrite is visible


def test_srgan_step_without_its_dead_gradients(gpu):
    """srgan_step(prune_dead_grads=True) skips the two gradient computations of the reference's iteration that nothing
    reads (G's in the D step, D's parameter gradients in the G step): parameters, Adam states and BatchNorm statistics
    after each step must be the ones of the faithful step (parameters and statistics bit for bit)."""
    pkg = _pkg()
    res = {}
    for prune in (False, True):
        G, D = pkg.SRGANGenerator(3, 64, 2), pkg.SRGANDiscriminator(3, 64, 32)
        fill.fill_module(G, 21, 0.5)
        fill.fill_module(D, 22, 0.5)
        G.to(gpu).train()
        D.to(gpu).train()
        gflat, dflat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
        g_opt = pkg.optim.make_optimizer("srgan_g", gflat, 1e-4)
        d_opt = pkg.optim.make_optimizer("srgan_d", dflat, 1e-4)
        lr, hr = B((4, 3, 8, 8), 83).to(gpu), B((4, 3, 32, 32), 84).to(gpu)
        step = pkg.trainers.srgan_step(G, D, g_opt, d_opt, prune_dead_grads=prune)
        losses = [tuple(float(v.detach()) for v in step(lr, hr)) for _ in range(3)]
        torch.cuda.synchronize()
        bn = torch.cat([torch.cat([m.running_mean, m.running_var]) for net in (G, D) for m in net.modules()
                        if isinstance(m, torch.nn.BatchNorm2d)])
        states = [getattr(o, k).clone() for o in (g_opt, d_opt) for k in ("buf", "exp_avg", "exp_avg_sq")
                  if getattr(o, k, None) is not None]
        res[prune] = tuple([[tuple(float(v) for v in l) for l in losses], gflat.data.clone(), dflat.data.clone(), bn,
                            gflat.grad.clone()] + states)
        assert all(p.requires_grad for p in D.parameters())
    assert res[True][0] == res[False][0]
    names = ["G params", "D params", "BatchNorm running statistics", "G gradients"] + ["optimizer state %d" % i for i in range(8)]
    for what, a, b in zip(names, res[True][1:], res[False][1:]):
        if what == "G gradients" or what.startswith("optimizer"):
            # (the weight gradients of a step are launched grouped by geometry and a group's split-K partition depends on
            #  how many layers share it: without D's dead records G's groups split differently -- last-bit differences)
            assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), what
        else:
            assert torch.equal(a, b), (what, float((a - b).abs().max()), float(b.abs().max()))


def test_srgan_step_is_its_segments_run_in_order(gpu):
    """trainers.srgan_step is the eager closure of trainers.srgan_segments: the closure, and the segments run by hand
    (in order, dp.exchange() behind every segment that has a dp) from equal starts, are the same code -- parameters,
    optimizer states, BatchNorm statistics, gradients and losses after two steps must be bit-equal.
    Shapes: bit equality of two runs needs a step that repeats itself bit for bit.  The gradient of a single-slope PReLU
    is summed with one float atomicAdd per block of 2048 elements (k_act_bwd<4>), in whatever order the blocks arrive: up
    to two blocks the sum does not depend on the order (a + b == b + a), from three on its last bit does -- at 64 filters
    and four 8x8 patches two runs of the SAME closure differ by 1 ulp in the three PReLU slopes' gradients and Adam
    moments (measured; nothing else differs).  8 filters and two 4x4 patches keep the largest PReLU output, the second
    upsampler's [2, 8, 16, 16], at two blocks."""
    pkg = _pkg()
    res = {}
    for mode in ("closure", "segments"):
        G, D = pkg.SRGANGenerator(3, 8, 1), pkg.SRGANDiscriminator(3, 8, 16)
        fill.fill_module(G, 31, 0.5)
        fill.fill_module(D, 32, 0.5)
        G.to(gpu).train()
        D.to(gpu).train()
        gflat, dflat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
        g_opt = pkg.optim.make_optimizer("srgan_g", gflat, 1e-4)
        d_opt = pkg.optim.make_optimizer("srgan_d", dflat, 1e-4)
        g_dp, d_dp = pkg.dp.DataParallel(gflat), pkg.dp.DataParallel(dflat)   # (no process group: inactive, exchange = flush)
        lr, hr = B((2, 3, 4, 4), 85).to(gpu), B((2, 3, 16, 16), 86).to(gpu)
        assert hr.shape[0] * 8 * hr.shape[2] * hr.shape[3] <= 2 * 2048   # (the largest PReLU output: two blocks)
        if mode == "closure":
            step = pkg.trainers.srgan_step(G, D, g_opt, d_opt, g_dp, d_dp)
        else:
            segments = pkg.trainers.srgan_segments(G, D, g_opt, d_opt, g_dp, d_dp)
            assert [dp for _, dp in segments] == [d_dp, g_dp, None]

            def step(*batch):
                out = None
                for fn, dp in segments:
                    out = fn(*batch)
                    if dp is not None:
                        dp.exchange()
                return out
        losses = [v.detach().clone() for _ in range(2) for v in step(lr, hr)]
        torch.cuda.synchronize()
        bn = [t for net in (G, D) for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)
              for t in (m.running_mean.clone(), m.running_var.clone())]
        states = [getattr(o, k).clone() for o in (g_opt, d_opt) for k in ("buf", "exp_avg", "exp_avg_sq", "step_dev")
                  if getattr(o, k, None) is not None]
        res[mode] = losses + [gflat.data.clone(), dflat.data.clone(), gflat.grad.clone(), dflat.grad.clone()] + bn + states
    assert len(res["closure"]) == len(res["segments"]) > 8
    for i, (a, b) in enumerate(zip(res["closure"], res["segments"])):
        assert torch.equal(a, b), i


@pytest.mark.parametrize("kind", ["edsr", "lapsrn", "srgan_d"])
def test_merged_slab_reductions_equal_per_group_reductions(gpu, kind):
    """ops.flush_wgrads runs the slab reductions of all weight-gradient launch groups of a backward pass as ONE launch
    (srk_wgrad_reduce_defer / _flush): same gradients, bit for bit, as every group reducing its own slabs -- EDSR (grouped
    bf16x3 launches, the few-channel kernels of the first / last conv, pixel-shuffled dy), LapSRN (shared weights: a second
    update of a queued dw forces a flush in between) and the SRGAN discriminator (strided convs: exact-fp32 kernels)."""
    pkg = _pkg()
    ops = pkg.ops
    from oracle import fill
    grads = []
    for merge in (True, False):
        if kind == "edsr":
            net = pkg.EDSRNet(3, 64, 4)
            x, t = fill.rand((4, 3, 16, 12), 61), fill.rand((4, 3, 64, 48), 62)
            loss_of = lambda out: ops.l1_loss(out, t.to(gpu))
        elif kind == "lapsrn":
            net = pkg.LapSRNNet(3, 64, 3)
            x, t = fill.rand((2, 3, 12, 12), 63), fill.rand((2, 3, 48, 48), 64)
            loss_of = lambda out: ops.charbonnier_loss(out[1], t.to(gpu))
        else:
            net = pkg.SRGANDiscriminator(3, 64, 32)
            x, t = fill.rand((4, 3, 32, 32), 65), fill.rand((4, 1), 66)
            loss_of = lambda out: ops.bce_loss(out, t.to(gpu))
        fill.fill_module(net, 9, 0.5)
        net.to(gpu).train()
        flat = pkg.optim.FlatParams(net)
        flat.zero_grad()
        flat.plan.pack()
        prev = ops.MERGE_REDUCES
        ops.MERGE_REDUCES = merge
        try:
            ops.backward(loss_of(net(x.to(gpu))))
        finally:
            ops.MERGE_REDUCES = prev
        torch.cuda.synchronize()
        grads.append({n: g.clone() for n, g in flat.named_grads().items()})
    assert max(float(g.abs().max()) for g in grads[0].values()) > 0
    for name, g in grads[0].items():
        if "convt_I" in name:   # LapSRN's 3 -> 3 image deconvs run the shape-agnostic kernel, which sums with float atomics
            assert rel_err(g, grads[1][name]) < 1e-5, name
        else:
            assert torch.equal(g, grads[1][name]), name
