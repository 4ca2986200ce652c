"""VESPCN on the device against its fp64 torch restatement (tests/vespcn_ref.py): the forward and every gradient of the
training loss, eval()'s padding, the train step eagerly and as a replayed graph, and main.py --model_name VESPCN.

Bars: the project's contract, outputs and losses 1e-4 max|ref|, gradients 1e-3 max|ref| (+ 1e-9 where the reference can
be 0).  The weights come from a fixed seed with last-layer biases that put the flows near +-0.3 .. 2.5 px, and the test
asserts on the REFERENCE's coordinates (coarse stage and total flow) that every one is at least 1e-4 from an integer: on
a cell boundary fp32 and fp64 may pick different cells (a 0.001-std init would put every sample there)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vespcn_ref as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (C, side, scale, seed): seeds chosen on the CPU for the margin asserted below
CONFIGS = [(1, 16, 2, 9), (3, 12, 3, 3)]


@pytest.fixture(scope="module")
def pkg(gpu):
    import pytorch_super_resolution_model_collection_amd as p
    from pytorch_super_resolution_model_collection_amd import models, ops, optim, sr_trainers, trainers   # noqa: F401
    return p


def init(net, seed):
    """Weights N(0, 0.5 / sqrt(fan_in)), small biases; the two flow heads' biases set the flow's size."""
    g = torch.Generator().manual_seed(seed)
    for name, p in net.named_parameters():
        if name.endswith("weight"):
            p.data.copy_(torch.randn(p.shape, generator=g) * (0.5 / math.sqrt(p[0].numel())))
        else:
            p.data.copy_(torch.randn(p.shape, generator=g) * 0.01)

    def head(bias, lo, hi, unit):
        mag = (lo + (hi - lo) * torch.rand(bias.shape, generator=g)) / unit
        sign = (torch.rand(bias.shape, generator=g) < 0.5).float() * 2 - 1
        bias.data.copy_(torch.atanh(mag) * sign)
    head(net.mc.coarse[4].conv.bias, 0.3, 2.0, net.mc.max_flow)
    head(net.mc.fine[4].conv.bias, 0.1, 0.5, net.mc.max_flow / 4)
    return net


def case(pkg, c, side, r, seed, n=2):
    net = init(pkg.models.VESPCNNet(c, 64, r, 8.0), seed)
    g = torch.Generator().manual_seed(100 + seed)
    frames = torch.rand(n, 3, c, side, side, generator=g)
    target = torch.rand(n, c, r * (side - 8), r * (side - 8), generator=g)
    return net, frames, target


def margin(*flows):
    worst = 1.0
    for f in flows:
        for u in V.coordinates(f.detach()):
            worst = min(worst, float((u - u.round()).abs().min()))
    return worst


def close(got, want, rel, what):
    want = want.detach().double()
    got = got.detach().cpu().double()
    bar = rel * float(want.abs().max()) + 1e-9
    err = float((got - want).abs().max())
    print("%-34s err %.3e bar %.3e" % (what, err, bar))
    assert err <= bar, (what, err, bar)


@pytest.mark.parametrize("c,side,r,seed", CONFIGS, ids=str)
def test_forward_and_all_gradients(pkg, gpu, c, side, r, seed):
    net, frames, target = case(pkg, c, side, r, seed)
    sd = {k: v.detach().double().requires_grad_(True) for k, v in net.state_dict().items()}
    sr, mc, flow, coarse = V.forward_terms(sd, frames.double(), r)
    assert margin(flow, coarse) >= 1e-4
    assert 0.2 <= float(flow.abs().max()) <= 3.0
    want = ((sr - target.double()) ** 2).mean() + 0.01 * mc + 0.001 * V.flow_huber(flow)
    want.backward()
    net = net.to(gpu).train()
    got_sr, got_mc, got_flow = net.forward_terms(frames.to(gpu))
    close(got_sr, sr, 1e-4, "sr")
    close(got_mc, mc, 1e-4, "mc")
    close(got_flow, flow, 1e-4, "flow")
    ops = pkg.ops
    loss = ops.loss_sum(ops.loss_sum(ops.mse_loss(got_sr, target.to(gpu)), got_mc, 1.0, 0.01), ops.flow_huber_loss(got_flow),
                        1.0, 0.001)
    close(loss, want, 1e-4, "loss")
    loss.backward()
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        close(p.grad, sd[name].grad, 1e-3, "d " + name)


def test_eval_pads_to_a_multiple_of_4(pkg, gpu):
    net, _, _ = case(pkg, 1, 16, 2, 9)
    frames = torch.rand(1, 3, 1, 18, 22, generator=torch.Generator().manual_seed(5))
    sd = {k: v.detach().double() for k, v in net.state_dict().items()}
    sr, _, flow, coarse = V.forward_terms(sd, V.pad4(frames.double()), 2)
    assert margin(flow, coarse) >= 1e-4
    want = sr[:, :, :2 * (18 - 8), :2 * (22 - 8)]
    net = net.to(gpu).eval()
    with torch.no_grad():
        got = net(frames.to(gpu))
    assert tuple(got.shape) == (1, 1, 20, 28)
    close(got, want, 1e-4, "eval 18 x 22")
    net.train()
    with pytest.raises(ValueError, match="not a multiple of 4"):
        net(frames.to(gpu))


def _train(pkg, gpu, graphed, steps=3):
    net, frames, target = case(pkg, 1, 16, 2, 9, n=4)
    net = net.to(gpu).train()
    flat, opt, dp, step = pkg.trainers.build("vespcn", net, 1e-3, mc_weight=0.01, flow_weight=0.001)
    assert dp is None and hasattr(step, "segments") and type(opt).__name__ == "Adam"
    batch = (frames.to(gpu), target.to(gpu))
    run = pkg.trainers.capture_step(step, batch, warmup=0, flats=[flat]) if graphed else step
    losses = [run(*batch).detach().clone() for _ in range(steps)]
    torch.cuda.synchronize()
    if graphed:
        run.close()
    return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}


def test_eager_and_replayed_steps_are_bit_equal(pkg, gpu):
    eager_losses, eager_sd = _train(pkg, gpu, False)
    graph_losses, graph_sd = _train(pkg, gpu, True)
    for a, b in zip(eager_losses, graph_losses):
        assert torch.equal(a, b)
    for k in eager_sd:
        assert torch.equal(eager_sd[k], graph_sd[k]), k
    assert float(eager_losses[-1]) < float(eager_losses[0])     # three Adam steps on one batch go down
    # the first loss is the restated one
    net, frames, target = case(pkg, 1, 16, 2, 9, n=4)
    sd = {k: v.detach().double() for k, v in net.state_dict().items()}
    close(eager_losses[0], V.loss(sd, frames.double(), target.double(), 2), 1e-4, "step loss")


def test_terms_are_refused_and_weights_checked(pkg, gpu):
    net = pkg.models.VESPCNNet(1, 64, 2).to(gpu)
    with pytest.raises(ValueError, match="ssim_weight: vespcn trains on MSE"):
        pkg.trainers.build("vespcn", net, 1e-3, ssim_weight=0.5)
    with pytest.raises(ValueError, match="mc_weight -1.0 is not a non-negative"):
        pkg.trainers.build("vespcn", net, 1e-3, mc_weight=-1.0)


def test_main_trains_on_synthetic_clips(gpu, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--model_name", "VESPCN", "--synthetic", "--num_epochs", "2",
           "--steps_per_epoch", "3", "--batch_size", "4", "--crop_size", "32", "--scale_factor", "2", "--num_channels", "1",
           "--save_dir", str(tmp_path), "--save_epochs", "1", "--mc_weight", "0.02"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Epoch: [ 2] avg loss:" in r.stdout
    assert os.path.exists(os.path.join(str(tmp_path), "VESPCN", "model", "VESPCN_param.pkl"))


def test_two_epochs_from_clip_folders(pkg, gpu, tmp_path):
    """data.ClipDataset through PatchLoader and the common trainer: 5-frame 40 x 40 PNG clips; a clip of identical frames
    gives three identical LR frames under the shared draw."""
    import argparse
    from PIL import Image
    from pytorch_super_resolution_model_collection_amd import data
    rng = np.random.RandomState(0)
    for clip in ("moving", "still"):
        os.makedirs(str(tmp_path / "data" / "clips" / clip))
        still = rng.randint(0, 256, (40, 40, 3), dtype=np.uint8)
        for i in range(5):
            img = still if clip == "still" else rng.randint(0, 256, (40, 40, 3), dtype=np.uint8)
            Image.fromarray(img).save(str(tmp_path / "data" / "clips" / clip / ("%02d.png" % i)))
    ds = data.get_clip_training_set(str(tmp_path / "data"), ["clips"], 32, 2, is_gray=False, device=gpu)
    assert len(ds) == 6
    frames, hr = ds[4]                                  # a `still` item
    torch.cuda.synchronize()
    assert tuple(frames.shape) == (3, 3, 16, 16) and tuple(hr.shape) == (3, 32, 32)
    assert torch.equal(frames[0], frames[1]) and torch.equal(frames[1], frames[2])
    frames, _ = ds[0]
    assert not torch.equal(frames[0], frames[1])
    args = argparse.Namespace(model_name="VESPCN", train_dataset=["clips"], test_dataset=[], crop_size=32, num_threads=2,
                              num_channels=3, scale_factor=2, num_epochs=2, save_epochs=2, batch_size=3, test_batch_size=1,
                              lr=1e-3, data_dir=str(tmp_path / "data"), save_dir=str(tmp_path / "out"), gpu_mode=True)
    t = pkg.sr_trainers.VESPCN(args)
    history = t.train()
    assert len(history) == 2 and all(np.isfinite(history)) and t.data_source == "folder"
    # test() walks the same clip folders: every frame once, with its real neighbours (the ends use themselves)
    t.test_dataset = ["clips"]
    psnrs = t.test()
    assert len(psnrs) == 10 and all(np.isfinite(float(p)) for p in psnrs)
    ts = data.get_clip_test_set(str(tmp_path / "data"), "clips", 2, device=gpu)
    assert len(ts) == 10 and ts.neighbours(0) == (0, (0, 0, 1)) and ts.neighbours(4) == (0, (3, 4, 4))
    frames, hr = ts[1]                                  # a `moving` frame between two others
    torch.cuda.synchronize()
    assert tuple(frames.shape) == (3, 3, 20, 20) and tuple(hr.shape) == (3, 40, 40)
    assert not torch.equal(frames[0], frames[1]) and not torch.equal(frames[1], frames[2])
    with_neighbours = t._forward(frames.unsqueeze(0).to(gpu))
    alone = t._forward(frames[1:2].to(gpu))             # a picture: its own neighbours
    assert tuple(with_neighbours.shape) == tuple(alone.shape) == (1, 3, 24, 24)
    assert not torch.equal(with_neighbours, alone)
    still, _ = ts[7]                                    # a `still` frame: the three LR frames are one picture
    assert torch.equal(t._forward(still.unsqueeze(0).to(gpu)), t._forward(still[1:2].to(gpu)))


TOL_STEP = 5e-4      # the bars tests/test_train_gpu.py holds a step against the fp32 CPU oracle to


def test_one_step_matches_the_fp32_cpu_oracle(pkg, gpu):
    """One eager step against the same step in fp32 torch on the CPU (tests/vespcn_ref.py, torch.optim.Adam): the loss
    within 5e-4; per parameter tensor the L2 norm within 5e-4 of it and the sum within 10 * 5e-4 of the norm."""
    net, frames, target = case(pkg, 1, 16, 2, 9, n=4)
    oracle = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    o_opt = torch.optim.Adam(list(oracle.values()), lr=1e-3)
    o_loss = V.loss(oracle, frames, target, 2)
    o_opt.zero_grad()
    o_loss.backward()
    o_opt.step()
    net = net.to(gpu).train()
    flat, opt, dp, step = pkg.trainers.build("vespcn", net, 1e-3)
    loss = float(step(frames.to(gpu), target.to(gpu)).detach())
    print("step loss %.8f oracle %.8f" % (loss, float(o_loss)))
    assert abs(loss - float(o_loss)) <= TOL_STEP * abs(float(o_loss))
    sd = net.state_dict()
    for name, p in oracle.items():
        want, got = p.detach().double(), sd[name].detach().double().cpu()
        l2 = float(want.pow(2).sum().sqrt())
        assert abs(float(got.pow(2).sum().sqrt()) - l2) <= TOL_STEP * max(l2, 1e-8), "L2 " + name
        assert abs(float(got.sum()) - float(want.sum())) <= 10 * TOL_STEP * max(l2, 1e-8), "sum " + name


def _trainer_run(pkg, save_dir, epochs, **extra):
    import argparse
    args = argparse.Namespace(model_name="VESPCN", train_dataset=[], test_dataset=[], crop_size=32, num_threads=1,
                              num_channels=1, scale_factor=2, num_epochs=epochs, save_epochs=1, batch_size=4, test_batch_size=1,
                              lr=1e-3, data_dir="", save_dir=str(save_dir), gpu_mode=True, synthetic=True, steps_per_epoch=3,
                              **extra)
    torch.manual_seed(7)
    t = pkg.sr_trainers.VESPCN(args)
    history = t.train()
    return history, {k: v.detach().clone() for k, v in t.model.state_dict().items()}


def test_eager_replayed_and_resumed_runs_are_bit_equal(pkg, gpu, tmp_path):
    """Three epochs through the common trainer: captured (the default), --eager, and two epochs continued with --resume."""
    hist, want = _trainer_run(pkg, tmp_path / "a", 3)
    hist_e, eager = _trainer_run(pkg, tmp_path / "e", 3, eager=True)
    _trainer_run(pkg, tmp_path / "r", 2)
    hist_r, resumed = _trainer_run(pkg, tmp_path / "r", 3, resume="auto")
    assert hist == hist_e == hist_r and len(hist) == 3
    for k in want:
        assert torch.equal(want[k], eager[k]), k
        assert torch.equal(want[k], resumed[k]), k
