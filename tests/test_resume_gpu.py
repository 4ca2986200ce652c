"""--resume on the MI355X: optimizer state round trips (every make_optimizer kind and TensorAdam), loading in place under a
captured graph, and trainers stopped at an epoch boundary and continued by a NEW trainer object against the
uninterrupted run.

Yardsticks are uninterrupted runs of the code as it is.  --eager runs the same kernels in the same order every step, and
for nets whose kernels have no order-dependent float atomics (ESPCN, VDSR, EDSR: ReLU only) two eager runs repeat bit for
bit; every bit-exact case asserts that first.  Kept out of the bit-exact cases: single-slope PReLU gradients above two
blocks and LapSRN's 3 -> 3 deconvolution (float atomics).  The default graphed mode is not bit-equal to eager (an eager
first step, then replays), so there the resumed run is held to 4 x the difference D between the uninterrupted graphed and
the uninterrupted eager run, measured in the test: a resumed run is another mix of eager and replayed steps, its deviations
are of the kind D samples once, and Adam turns last-bit differences into +-lr flips.  D == 0 demands bit equality."""
import contextlib
import os
import shutil

import pytest
import torch

from oracle import fill

pytestmark = pytest.mark.gpu
B = fill.rand


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


# ---- 1. optimizer round trip ---------------------------------------------------------------------------------------------
# Seeded gradients written into the flat gradient buffer: the optimizer kernels are the only thing that runs, so every
# kind repeats bit for bit whatever its family's backward kernels do.
KINDS = {
    "srcnn": lambda pkg: pkg.SRCNNNet(3, 8),
    "fsrcnn": lambda pkg: pkg.FSRCNNNet(3, 2, 8, 4, 1),
    "vdsr": lambda pkg: pkg.VDSRNet(3, 8, 2),
    "espcn": lambda pkg: pkg.ESPCNNet(3, 8, 2),
    "lapsrn": lambda pkg: pkg.LapSRNNet(3, 8, 2),
    "drcn": lambda pkg: pkg.DRCNNet(3, 8, 2),
    "edsr": lambda pkg: pkg.EDSRNet(3, 8, 1),
    "srgan_g": lambda pkg: pkg.SRGANGenerator(3, 8, 1),
    "srgan_d": lambda pkg: pkg.SRGANDiscriminator(3, 8, 16),
}
STATELESS = ("srcnn",)     # plain SGD: nothing but the rate


def _make(gpu, kind, seed, lr, ema_decay):
    pkg = _pkg()
    net = KINDS[kind](pkg)
    fill.fill_module(net, seed)
    net.to(gpu).train()
    flat = pkg.optim.FlatParams(net)
    return net, flat, pkg.optim.make_optimizer(kind, flat, lr, ema_decay=ema_decay)


def _opt_tensors(opt):
    """Every device tensor of an optimizer's state, by name."""
    out = {"params": opt.flat.data, "lr": opt.lr_dev}
    for k in ("buf", "exp_avg", "exp_avg_sq", "step_dev", "ema"):
        if getattr(opt, k, None) is not None:
            out[k] = getattr(opt, k)
    return out


def _steps(opt, first, count):
    """Steps first .. first + count - 1 (gradient of step s: seed 1000 + s; the rate halves in front of step 2).  The
    alignment padding between parameters gets no gradient, as in training: nothing there is state."""
    f = opt.flat
    for s in range(first, first + count):
        if s == 2:
            opt.param_groups[0]["lr"] = opt.param_groups[0]["lr"] / 2
        g = B((f.numel,), 1000 + s).to(f.grad.device)
        f.grad.zero_()
        for p, o in zip(f.params, f.offsets):
            f.grad[o:o + p.numel()].copy_(g[o:o + p.numel()])
        opt.step()
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in _opt_tensors(opt).items()}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_optimizer_round_trip(gpu, kind, tmp_path):
    net_a, flat_a, opt_a = _make(gpu, kind, 1, 1e-2, 0.9)
    _steps(opt_a, 0, 3)
    name = str(tmp_path / "opt.pkl")
    torch.save({"opt": opt_a.state_dict(), "model": {k: v.cpu().clone() for k, v in net_a.state_dict().items()}}, name)
    want = _steps(opt_a, 3, 3)
    saved = torch.load(name, map_location="cpu", weights_only=True)
    # per-parameter state under the model's own names, in the parameters' shapes; padding is not state
    shapes = dict((n, tuple(p.shape)) for n, p in zip(flat_a.names, flat_a.params))
    assert sorted(saved["opt"]["state"]) == sorted(shapes) == sorted(saved["opt"]["ema"]["params"])
    for n, per in saved["opt"]["state"].items():
        assert all(tuple(t.shape) == shapes[n] for t in per.values())
    if "step_dev" in want:
        assert saved["opt"]["step"] == 3

    # a fresh model (another fill) and optimizer (another rate): weights and state loaded -> steps 4..6 bit for bit
    net_b, flat_b, opt_b = _make(gpu, kind, 2, 3e-2, 0.9)
    ptrs = {k: v.data_ptr() for k, v in _opt_tensors(opt_b).items()}
    net_b.load_state_dict(saved["model"])
    opt_b.load_state_dict(saved["opt"])
    assert {k: v.data_ptr() for k, v in _opt_tensors(opt_b).items()} == ptrs      # in place
    assert opt_b.param_groups[0]["lr"] == opt_a.param_groups[0]["lr"]
    got = _steps(opt_b, 3, 3)
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), (kind, k)

    # the weights alone (same rate, so that only the state is missing): not the same run, unless there is no state
    net_c, flat_c, opt_c = _make(gpu, kind, 2, opt_a.param_groups[0]["lr"], 0.0)
    net_c.load_state_dict(saved["model"])
    got = _steps(opt_c, 3, 3)
    assert torch.equal(got["params"], want["params"]) == (kind in STATELESS), kind


def test_tensor_adam_round_trip(gpu):
    pkg = _pkg()

    def make(seed, lr):
        t = B((16,), seed, 0.2, 1.0).to(gpu).requires_grad_(True)
        return t, pkg.optim.TensorAdam(t, lr)

    def steps(t, opt, first):
        for s in range(first, first + 3):
            if s == 2:
                opt.param_groups[0]["lr"] = opt.param_groups[0]["lr"] / 10
            opt.grad.copy_(B((16,), 2000 + s).to(gpu))
            opt.step()
        torch.cuda.synchronize()
        return [x.detach().clone() for x in (t, opt.exp_avg, opt.exp_avg_sq, opt.step_dev, opt.lr_dev)]

    t_a, opt_a = make(1, 1e-2)
    steps(t_a, opt_a, 0)
    sd, w = opt_a.state_dict(), t_a.detach().cpu().clone()
    assert sd["step"] == 3 and sd["state"]["exp_avg"].shape == (16,) and not sd["state"]["exp_avg"].is_cuda
    want = steps(t_a, opt_a, 3)
    t_b, opt_b = make(2, 5e-2)
    ptrs = [x.data_ptr() for x in (opt_b.exp_avg, opt_b.exp_avg_sq, opt_b.step_dev, opt_b.lr_dev)]
    with torch.no_grad():
        t_b.copy_(w)
    opt_b.load_state_dict(sd)
    assert ptrs == [x.data_ptr() for x in (opt_b.exp_avg, opt_b.exp_avg_sq, opt_b.step_dev, opt_b.lr_dev)]
    for a, b in zip(steps(t_b, opt_b, 3), want):
        assert torch.equal(a, b)
    t_c, opt_c = make(2, opt_a.param_groups[0]["lr"])
    with torch.no_grad():
        t_c.copy_(w)
    assert not torch.equal(steps(t_c, opt_c, 3)[0], want[0])
    with pytest.raises(ValueError, match="adam"):
        opt_b.load_state_dict(dict(sd, kind="adam"))


def test_load_state_dict_refuses_what_does_not_fit(gpu, capsys):
    pkg = _pkg()
    net, flat, opt = _make(gpu, "espcn", 1, 1e-3, 0.9)
    _steps(opt, 0, 1)
    sd = opt.state_dict()
    # another kind
    net_s, flat_s, sgd = _make(gpu, "vdsr", 1, 1e-3, 0.0)
    with pytest.raises(ValueError, match="adam"):
        sgd.load_state_dict(sd)
    # another name set: the first offender is named
    first = flat.names[0]
    less = dict(sd, state={k: v for k, v in sd["state"].items() if k != first})
    with pytest.raises(ValueError, match=first.replace(".", r"\.")):
        opt.load_state_dict(less)
    more = dict(sd, state=dict(sd["state"], stranger=sd["state"][first]))
    with pytest.raises(ValueError, match="stranger"):
        opt.load_state_dict(more)
    # another shape
    bad = dict(sd, state=dict(sd["state"]))
    bad["state"][first] = {k: v.reshape(-1) for k, v in sd["state"][first].items()}
    with pytest.raises(ValueError, match=first.replace(".", r"\.")):
        opt.load_state_dict(bad)
    # a state with EMA into an optimizer without: ignored, and said; a state without into one with: ema_reset()
    net_n, flat_n, plain = _make(gpu, "espcn", 1, 1e-3, 0.0)
    capsys.readouterr()
    plain.load_state_dict(sd)
    assert "EMA" in capsys.readouterr().out and plain.ema is None
    no_ema = {k: v for k, v in sd.items() if k != "ema"}
    assert not torch.equal(opt.ema, flat.data)
    opt.load_state_dict(no_ema)
    assert torch.equal(opt.ema, flat.data)


# ---- 2. in place under a graph -------------------------------------------------------------------------------------------
def test_load_in_place_under_a_captured_graph(gpu):
    pkg = _pkg()
    net = pkg.EDSRNet(3, 64, 2)
    fill.fill_module(net, 7, 0.5)
    net.to(gpu).train()
    flat, opt, dp, step = pkg.trainers.build("edsr", net, 1e-3, ema_decay=0.9)
    batches = [(B((2, 3, 8, 8), 70 + i).to(gpu), B((2, 3, 32, 32), 80 + i).to(gpu)) for i in range(5)]
    step(*batches[0])
    graph = pkg.trainers.capture_step(step, batches[0], warmup=0, flats=[flat])
    for b in batches[1:3]:
        graph(*b)
    torch.cuda.synchronize()
    snap_opt = opt.state_dict()
    snap_model = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    assert snap_opt["step"] == 3
    tensors = dict(_opt_tensors(opt), grad=flat.grad, scale=opt.scale_dev)
    ptrs = {k: v.data_ptr() for k, v in tensors.items()}
    pptrs = [p.data_ptr() for p in net.parameters()]

    def two_more():
        for b in batches[3:5]:
            graph(*b)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in _opt_tensors(opt).items()}

    a = two_more()
    net.load_state_dict(snap_model)
    opt.load_state_dict(snap_opt)
    assert int(opt.step_dev[0]) == 3 and int(opt.step_dev[1]) == 0
    b = two_more()
    graph.close()
    assert int(opt.step_dev[0]) == 5
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert {k: v.data_ptr() for k, v in tensors.items()} == ptrs
    assert [p.data_ptr() for p in net.parameters()] == pptrs


# ---- 3 / 4. trainers -----------------------------------------------------------------------------------------------------
MODELS = {"ESPCN": ["--crop_size", "48"], "VDSR": ["--crop_size", "17"], "EDSR": ["--crop_size", "32"]}


@contextlib.contextmanager
def _decay_every_two_epochs(kind, table=None):
    """The rate halves at the top of epochs 2 and 4 (as tests/test_train_gpu.py patches it): a run of 4 epochs stopped
    after 2 has one decay in front of the interruption, stored in the rate, and one behind it."""
    from pytorch_super_resolution_model_collection_amd import sr_trainers
    table = sr_trainers.LR_DECAY if table is None else table
    old = dict(table)
    table[kind] = (2, 2.0)
    try:
        yield
    finally:
        table.clear()
        table.update(old)


def _args(name, save_dir, epochs, *extra):
    import main as cli
    return cli.parse_args(["--model_name", name, "--num_epochs", str(epochs), "--batch_size", "2", "--synthetic",
                           "--steps_per_epoch", "2", "--lr", "1e-3", "--save_dir", str(save_dir)] + list(extra))


def _run(cls, args, seed=0):
    torch.manual_seed(seed)
    t = cls(args)
    hist = t.train()
    torch.cuda.synchronize()
    return t, hist


def _trainer_state(t):
    out = {k: v.detach().clone() for k, v in _opt_tensors(t.optimizer).items()}
    out.update(("model." + k, v.detach().clone()) for k, v in t.model.state_dict().items())
    return out


def _weights_only(cls):
    """The trainer continued from the weights of the state file alone: what --resume would be without the rest."""
    class WeightsOnly(cls):
        def load_training_state(self, state, loader=None):
            self.model.load_state_dict(state["modules"]["model"])
            return int(state["epochs_done"]), list(state["history"])
    return WeightsOnly


@pytest.mark.parametrize("name", sorted(MODELS))
def test_trainer_resumes_bit_exactly_eager(gpu, tmp_path, name):
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    cls, extra = TRAINERS[name], MODELS[name] + ["--eager", "--ema_decay", "0.9"]
    with _decay_every_two_epochs(name.lower()):
        a, hist_a = _run(cls, _args(name, tmp_path / "a", 4, "--save_epochs", "10", *extra))
        a2, hist_a2 = _run(cls, _args(name, tmp_path / "a2", 4, "--save_epochs", "10", *extra))
        want, again = _trainer_state(a), _trainer_state(a2)
        assert hist_a == hist_a2 and all(torch.equal(want[k], again[k]) for k in want), "%s: two eager runs differ" % name
        assert a.optimizer.param_groups[0]["lr"] == 1e-3 / 4
        # 2 epochs, then a new trainer object continues to 4 (another seed: nothing of the fresh initialisation survives)
        b1, hist_b1 = _run(cls, _args(name, tmp_path / "b", 2, "--save_epochs", "2", *extra))
        assert hist_b1 == hist_a[:2]
        state_file = os.path.join(str(tmp_path / "b"), name, "model", name + "_train_state.pkl")
        assert os.path.exists(state_file) and not os.path.exists(state_file + ".tmp")
        after_two = str(tmp_path / "after_two.pkl")
        shutil.copy(state_file, after_two)
        b2, hist_b2 = _run(cls, _args(name, tmp_path / "b", 4, "--save_epochs", "10", "--resume", *extra), seed=123)
        got = _trainer_state(b2)
        assert hist_b2 == hist_a
        assert sorted(got) == sorted(want) and "ema" in want
        for k in want:
            assert torch.equal(got[k], want[k]), (name, k)
        assert b2.optimizer.param_groups[0]["lr"] == a.optimizer.param_groups[0]["lr"]
        # the final state file says so
        done = torch.load(state_file, map_location="cpu", weights_only=True)
        assert done["epochs_done"] == 4 and done["history"] == hist_a
        # from the weights alone the run is another one
        c, hist_c = _run(_weights_only(cls), _args(name, tmp_path / "c", 4, "--save_epochs", "10", "--resume", after_two,
                                                   *extra), seed=123)
        assert not torch.equal(c.flat.data, a.flat.data), name


def test_resume_errors(gpu, tmp_path):
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    with pytest.raises(FileNotFoundError, match="resume"):
        TRAINERS["ESPCN"](_args("ESPCN", tmp_path / "none", 1, "--crop_size", "48", "--resume")).train()
    _run(TRAINERS["ESPCN"], _args("ESPCN", tmp_path / "e", 1, "--crop_size", "48", "--eager"))
    state_file = os.path.join(str(tmp_path / "e"), "ESPCN", "model", "ESPCN_train_state.pkl")
    with pytest.raises(ValueError, match="model_name"):
        TRAINERS["VDSR"](_args("VDSR", tmp_path / "v", 1, "--crop_size", "17", "--resume", state_file)).train()
    with pytest.raises(ValueError, match="num_channels"):
        TRAINERS["ESPCN"](_args("ESPCN", tmp_path / "e1", 1, "--crop_size", "48", "--num_channels", "1", "--resume",
                                state_file)).train()
    with pytest.raises(ValueError, match="scale_factor"):
        TRAINERS["ESPCN"](_args("ESPCN", tmp_path / "e2", 1, "--crop_size", "48", "--scale_factor", "2", "--resume",
                                state_file)).train()
    args = _args("DRCN", tmp_path / "d", 1, "--crop_size", "16")
    args.ema_decay = 0.9                      # (the command line refuses it before a trainer sees it)
    with pytest.raises(ValueError, match="ema_decay"):
        TRAINERS["DRCN"](args)


def test_resume_with_another_rate_keeps_the_stored_one(gpu, tmp_path, capsys):
    """Another --lr or --batch_size is allowed: the stored rate wins, and one printed line says so."""
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    _run(TRAINERS["ESPCN"], _args("ESPCN", tmp_path, 1, "--crop_size", "48", "--eager"))
    capsys.readouterr()
    args = _args("ESPCN", tmp_path, 2, "--crop_size", "48", "--eager", "--resume")
    args.lr, args.batch_size = 5e-2, 4
    t, hist = _run(TRAINERS["ESPCN"], args)
    said = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Resumed after epoch 1")]
    assert len(said) == 1 and "stored learning rate 0.001" in said[0] and "batch_size 2 -> 4" in said[0], said
    assert len(hist) == 2 and t.optimizer.param_groups[0]["lr"] == 1e-3
    assert float(t.optimizer.lr_dev) == float(torch.tensor(1e-3, dtype=torch.float32))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_trainer_resumes_graphed(gpu, tmp_path, name):
    """The default mode (the first step of a shape eager, then replays); see the module docstring for the bar."""
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    cls, extra = TRAINERS[name], MODELS[name]
    with _decay_every_two_epochs(name.lower()):
        g, hist_g = _run(cls, _args(name, tmp_path / "g", 4, "--save_epochs", "10", *extra))
        e, hist_e = _run(cls, _args(name, tmp_path / "e", 4, "--save_epochs", "10", "--eager", *extra))
        r1, hist_r1 = _run(cls, _args(name, tmp_path / "r", 2, "--save_epochs", "2", *extra))
        r, hist_r = _run(cls, _args(name, tmp_path / "r", 4, "--save_epochs", "10", "--resume", *extra), seed=123)
    D = float((g.flat.data - e.flat.data).abs().max())
    diff = float((r.flat.data - g.flat.data).abs().max())
    print("resume parity %s: D = max|graphed - eager| = %.9g, max|resumed graphed - graphed| = %.9g" % (name, D, diff))
    assert len(hist_r) == 4 and hist_r[:2] == hist_r1      # the stored history, then the new epochs
    if D == 0:
        assert torch.equal(r.flat.data, g.flat.data)
    else:
        assert diff <= 4 * D, (name, diff, D)


# ---- 5. SRGAN and DRCN ---------------------------------------------------------------------------------------------------
def _snapshots(cls):
    """The trainer, keeping a copy of every state file it writes: <save_dir>/snap_<phase>_<epochs done>.pkl."""
    class Snapshots(cls):
        def _write_state(self, state):
            super(Snapshots, self)._write_state(state)
            torch.save(state, os.path.join(self.save_dir, "snap_%s_%d.pkl" % (state.get("phase", "train"),
                                                                              state["epochs_done"])))
    return Snapshots


def test_srgan_resumes_in_either_phase(gpu, tmp_path):
    """8 filters, one residual block, 16 x 16 crops in batches of 2: every single-slope PReLU gradient stays at two blocks
    (tests/test_train_gpu.py::test_srgan_step_is_its_segments_run_in_order), so an eager run repeats bit for bit."""
    pkg = _pkg()
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS

    class Small(_snapshots(TRAINERS["SRGAN"])):
        def build_model(self):
            self.G = pkg.SRGANGenerator(self.num_channels, 8, 1)
            self.D = pkg.SRGANDiscriminator(self.num_channels, 8, self.crop_size)
            return self.G

    extra = ["--crop_size", "16", "--eager", "--epoch_pretrain", "2", "--save_epochs", "1", "--ema_decay", "0.9"]

    def final(t, hist):
        out = {"G." + k: v.detach().clone() for k, v in t.G.state_dict().items()}
        out.update(("D." + k, v.detach().clone()) for k, v in t.D.state_dict().items())
        out.update(("g_opt." + k, v.clone()) for k, v in _opt_tensors(t.g_opt).items())
        out.update(("d_opt." + k, v.clone()) for k, v in _opt_tensors(t.d_opt).items())
        return out, hist, t.phase

    with _decay_every_two_epochs("srgan"):
        a, hist_a = _run(Small, _args("SRGAN", tmp_path / "a", 3, *extra))
        a2, hist_a2 = _run(Small, _args("SRGAN", tmp_path / "a2", 3, *extra))
        want, again = final(a, hist_a), final(a2, hist_a2)
        assert want[1:] == again[1:] and all(torch.equal(want[0][k], again[0][k]) for k in want[0]), "two eager runs differ"
        assert want[2] == "adversarial" and len(hist_a) == 3 and "g_opt.ema" in want[0] and "d_opt.ema" not in want[0]
        mdir = os.path.join(str(tmp_path / "a"), "SRGAN", "model")
        assert os.path.exists(os.path.join(mdir, "SRGAN_G_param_pretrain_ema.pkl"))
        # G only: the pre-trained one and epochs 1, 2, 3 (the final file has epoch 3's name)
        assert len([f for f in os.listdir(mdir) if f.endswith("_ema.pkl")]) == 1 + 3
        for snap, phase in (("snap_pretrain_1.pkl", "pretrain"), ("snap_adversarial_0.pkl", "adversarial"),
                            ("snap_adversarial_2.pkl", "adversarial")):
            path = os.path.join(str(tmp_path / "a"), "SRGAN", snap)
            assert torch.load(path, map_location="cpu", weights_only=True)["phase"] == phase
            b, hist_b = _run(Small, _args("SRGAN", tmp_path / ("b_" + snap), 3, "--resume", path, *extra), seed=123)
            got = final(b, hist_b)
            assert got[1:] == want[1:], snap
            for k in want[0]:
                assert torch.equal(got[0][k], want[0][k]), (snap, k)


def test_drcn_resumes_with_its_alpha_and_w(gpu, tmp_path):
    """32 filters, 4 recursions, 16 x 16 crops: two uninterrupted eager runs repeat bit for bit (asserted first), so the
    resumed one must too."""
    from pytorch_super_resolution_model_collection_amd import sr_trainers
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS

    class Small(_snapshots(TRAINERS["DRCN"])):
        base_filter, num_recursions = 32, 4

    extra = ["--crop_size", "16", "--eager", "--save_epochs", "1"]

    def final(t):
        out = {"model." + k: v.detach().clone() for k, v in t.model.state_dict().items()}
        out["w"] = t.model.w.detach().clone()
        out.update(("opt." + k, v.clone()) for k, v in _opt_tensors(t.optimizer).items())
        out.update(("w_opt." + k, getattr(t.w_optimizer, k).clone()) for k in ("exp_avg", "exp_avg_sq", "step_dev", "lr_dev"))
        return out

    with _decay_every_two_epochs("drcn", sr_trainers.LR_DECAY_DRCN):
        a, hist_a = _run(Small, _args("DRCN", tmp_path / "a", 4, *extra))
        a2, hist_a2 = _run(Small, _args("DRCN", tmp_path / "a2", 4, *extra))
        want, again = final(a), final(a2)
        assert hist_a == hist_a2 and all(torch.equal(want[k], again[k]) for k in want), "two eager runs differ"
        path = os.path.join(str(tmp_path / "a"), "DRCN", "snap_train_2.pkl")
        state = torch.load(path, map_location="cpu", weights_only=True)
        assert abs(state["loss_alpha"] - 0.92) < 1e-12      # alpha has moved: two epochs of 1 / 25 each
        assert state["w"].shape == (4,) and sorted(state["optimizers"]) == ["optimizer", "w_optimizer"]
        b, hist_b = _run(Small, _args("DRCN", tmp_path / "b", 4, "--resume", path, *extra), seed=123)
    got = final(b)
    assert hist_b == hist_a and b.loss_alpha == a.loss_alpha
    assert b.optimizer.param_groups[0]["lr"] == a.optimizer.param_groups[0]["lr"] == 1e-3 / 4
    assert b.w_optimizer.param_groups[0]["lr"] == a.w_optimizer.param_groups[0]["lr"] == 1e-3 / 4
    assert not torch.equal(want["w"], torch.full_like(want["w"], 0.25))      # (w trained)
    for k in want:
        assert torch.equal(got[k], want[k]), k
