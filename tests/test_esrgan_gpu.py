"""ESRGAN on the GPU: RRDBNet against the fp64 plain-torch restatement of tests/esrgan_ref.py (output and every parameter
gradient), one pre-training and one adversarial step against the fp32 CPU oracle step (the same terms in the same order,
BatchNorm statistics included), the eager step against its captured graph, --resume in both phases, network
interpolation, and test().

Bars: the forward within 1e-4, gradients within 1e-3 of fp64, relative to the reference tensor's maximum; the steps under
the bars tests/test_train_gpu.py holds the SRGAN step to (losses within 5e-4; per parameter tensor the L2 norm within
5e-4 of it and the sum within 10 * 5e-4 of the norm)."""
import os

import numpy as np
import pytest
import torch

import esrgan_ref as E
import perceptual_ref as P
import rdn_ref as R
from conftest import rel_err
from oracle import fill

pytestmark = pytest.mark.gpu

TOL_FWD, TOL_GRAD, TOL_STEP = 1e-4, 1e-3, 5e-4
VGG_SEED = 78


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def vgg_file(tmp_path_factory):
    """A filled vgg19.features[:35] (conv5_4 before its ReLU) under torchvision's names, written once."""
    path = str(tmp_path_factory.mktemp("vgg") / "vgg19_head34.pth")
    torch.save(P.filled_head(34, VGG_SEED)[2], path)
    return path


def test_net_matches_fp64(gpu):
    pkg = _pkg()
    ctor = (3, 32, 2, 16)
    net = pkg.RRDBNet(*ctor, scale_factor=4)
    fill.fill_module(net, 3, 0.7)
    net.to(gpu).train()
    ref = E.ref_net_like(net, *ctor)
    x, t = fill.rand((2, 3, 12, 12), 8), fill.rand((2, 3, 48, 48), 9)
    want = ref(x.double())
    torch.nn.functional.l1_loss(want, t.double()).backward()
    got = net(x.to(gpu))
    pkg.ops.l1_loss(got, t.to(gpu)).backward()
    err = R.worst(got.detach(), want.detach())
    print("RRDBNet %s forward: worst %.3e of max |ref|" % (ctor, err))
    assert got.shape == want.shape and err <= TOL_FWD
    wg = dict(ref.named_parameters())
    worst = ("", 0.0)
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        e = R.worst(p.grad, wg[name].grad)
        worst = max(worst, (name, e), key=lambda v: v[1])
        assert e <= TOL_GRAD, (name, e)
    print("RRDBNet %s gradients: worst %.3e of max |ref| (%s)" % (ctor, worst[1], worst[0]))
    net.eval()
    with torch.no_grad():
        assert R.worst(net(x.to(gpu)), want.detach()) <= TOL_FWD


def _check_params(net, oracle, tag):
    sd = net.state_dict()
    for n, p in oracle.state_dict().items():
        if not p.is_floating_point():
            continue
        want, t = p.detach().double(), sd[n].detach().double().cpu()
        l2 = float(want.pow(2).sum().sqrt())
        assert abs(float(t.pow(2).sum().sqrt()) - l2) <= TOL_STEP * max(l2, 1e-8), "%s L2 %s" % (tag, n)
        assert abs(float(t.sum()) - float(want.sum())) <= 10 * TOL_STEP * max(l2, 1e-8), "%s sum %s" % (tag, n)


def _nets(pkg, gpu, nf=64, nb=1, gc=32, bf=64):
    G, D = pkg.RRDBNet(3, nf, nb, gc, 4), pkg.ESRGANDiscriminator(3, bf, 32)
    fill.fill_module(G, 5, 0.7)
    fill.fill_module(D, 6, 1.0)
    return G.to(gpu).train(), D.to(gpu).train()


def _extractor(pkg, gpu):
    return pkg.FeatureExtractor(feature_layer=34).load_vgg19(P.filled_head(34, VGG_SEED)[2]).to(gpu)


def test_steps_match_the_cpu_oracle(gpu):
    """Batch 4, nb = 1, 8 x 8 LR, 32 x 32 HR: the smallest size at which the discriminator's four stride-2 stages and the
    VGG head's pools still leave a map.  One L1 pre-training step, then one adversarial step, both at lr 1e-4."""
    pkg = _pkg()
    G, D = _nets(pkg, gpu)
    oG = E.RefRRDBNet(3, 64, 1, 32)
    oG.load_state_dict({k: v.detach().cpu() for k, v in G.state_dict().items()})
    oD = E.ref_discriminator(3, 64, 32)
    oD.load_state_dict({k: v.detach().cpu() for k, v in D.state_dict().items()})
    oG.train()
    oD.train()
    lr_img, hr_img = fill.rand((4, 3, 8, 8), 120), fill.rand((4, 3, 32, 32), 130)
    g_flat, d_flat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
    g_opt = pkg.optim.make_optimizer("esrgan_g", g_flat, 1e-4)
    d_opt = pkg.optim.make_optimizer("esrgan_d", d_flat, 1e-4)
    assert isinstance(g_opt, pkg.optim.Adam) and isinstance(d_opt, pkg.optim.Adam)
    og_opt = torch.optim.Adam(oG.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    od_opt = torch.optim.Adam(oD.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    # phase 1
    pre = float(pkg.trainers.l1_step(G, g_opt)(lr_img.to(gpu), hr_img.to(gpu)).detach())
    opre = E.oracle_pretrain_step(oG, og_opt, lr_img, hr_img)
    print("pretrain loss %.8f oracle %.8f" % (pre, opre))
    assert abs(pre - opre) <= TOL_STEP * abs(opre)
    _check_params(G, oG, "pretrain G")
    # phase 2
    step = pkg.trainers.esrgan_step(G, D, g_opt, d_opt, _extractor(pkg, gpu))
    d_loss, g_loss = (float(v.detach()) for v in step(lr_img.to(gpu), hr_img.to(gpu)))
    od, og = E.oracle_adversarial_step(oG, oD, og_opt, od_opt, P.filled_head(34, VGG_SEED)[0], P.vnorm, lr_img, hr_img)
    print("adversarial d_loss %.8f oracle %.8f  g_loss %.8f oracle %.8f" % (d_loss, od, g_loss, og))
    assert rel_err(np.array([d_loss, g_loss]), np.array([od, og])) < TOL_STEP
    _check_params(G, oG, "adversarial G")
    _check_params(D, oD, "adversarial D")      # (running statistics included: four training-mode forwards)
    assert all(p.requires_grad for p in D.parameters())


def test_graphed_step_equals_eager(gpu):
    """Two steps of trainers.esrgan_step: replayed from a captured graph they leave the eager run's parameters, optimizer
    states and BatchNorm statistics, bit for bit."""
    pkg = _pkg()
    batches = [(fill.rand((4, 3, 8, 8), 50 + i).to(gpu), fill.rand((4, 3, 32, 32), 60 + i).to(gpu)) for i in range(2)]
    fe = _extractor(pkg, gpu)

    def make():
        G, D = _nets(pkg, gpu, 32, 1, 16, 8)
        g_flat, d_flat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
        g_opt = pkg.optim.make_optimizer("esrgan_g", g_flat, 1e-3)
        d_opt = pkg.optim.make_optimizer("esrgan_d", d_flat, 1e-3)
        return G, D, g_flat, d_flat, g_opt, d_opt, pkg.trainers.esrgan_step(G, D, g_opt, d_opt, fe)

    def state(G, D, g_opt, d_opt):
        out = [g_opt.flat.data, d_opt.flat.data, g_opt.exp_avg, g_opt.exp_avg_sq, d_opt.exp_avg, d_opt.exp_avg_sq]
        return out + [b for b in D.buffers() if b.is_floating_point()]

    G, D, g_flat, d_flat, g_opt, d_opt, step = make()
    losses_a = [[float(v.detach()) for v in step(*b)] for b in batches]
    want = [t.clone() for t in state(G, D, g_opt, d_opt)]
    G, D, g_flat, d_flat, g_opt, d_opt, step = make()
    graph = pkg.trainers.capture_step(step, batches[0], warmup=0, flats=[g_flat, d_flat])
    losses_b = [[float(v.detach()) for v in graph(*batches[0])]]     # the capture itself ran nothing
    losses_b.append([float(v.detach()) for v in graph(*batches[1])])
    graph.close()
    assert losses_a == losses_b
    for i, (a, b) in enumerate(zip(want, state(G, D, g_opt, d_opt))):
        assert torch.equal(a, b), i


def _args(save_dir, epochs, vgg_file, *extra):
    import main as cli
    return cli.parse_args(["--model_name", "ESRGAN", "--rrdb_blocks", "1", "--rrdb_growth", "16", "--crop_size", "32",
                           "--num_epochs", str(epochs), "--batch_size", "2", "--synthetic", "--steps_per_epoch", "2",
                           "--lr", "1e-3", "--save_dir", str(save_dir), "--vgg_weights", vgg_file] + list(extra))


def _small(pkg):
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS

    class Small(TRAINERS["ESRGAN"]):
        """16 trunk channels and an 8-filter discriminator; every state file kept as snap_<phase>_<epochs>.pkl."""

        def build_model(self):
            self.G = pkg.RRDBNet(self.num_channels, 16, self.blocks, self.growth, self.scale_factor)
            self.D = pkg.ESRGANDiscriminator(self.num_channels, 8, self.crop_size)
            return self.G

        def _write_state(self, state):
            super(Small, self)._write_state(state)
            torch.save(state, os.path.join(self.save_dir, "snap_%s_%d.pkl" % (state.get("phase", "train"),
                                                                              state["epochs_done"])))
    return Small


def _train(cls, args, seed=0):
    torch.manual_seed(seed)
    t = cls(args)
    hist = t.train()
    torch.cuda.synchronize()
    return t, hist


def _final(t):
    out = {"G." + k: v.detach().clone() for k, v in t.G.state_dict().items()}
    out.update(("D." + k, v.detach().clone()) for k, v in t.D.state_dict().items())
    for name, o in (("g_opt", t.g_opt), ("d_opt", t.d_opt)):
        out.update({"%s.exp_avg" % name: o.exp_avg.clone(), "%s.exp_avg_sq" % name: o.exp_avg_sq.clone()})
    out["g_opt.ema"] = t.g_opt.ema.clone()
    return out


@pytest.fixture(scope="module")
def trained(gpu, tmp_path_factory, vgg_file):
    """One eager run of the small trainer: 2 pre-training epochs, 2 adversarial ones, a state file at every boundary."""
    root = tmp_path_factory.mktemp("esrgan")
    extra = ["--eager", "--epoch_pretrain", "2", "--save_epochs", "1", "--ema_decay", "0.9"]
    t, hist = _train(_small(_pkg()), _args(root / "a", 2, vgg_file, *extra))
    return root, extra, t, hist


def test_trainer_runs_both_phases(trained):
    root, extra, t, hist = trained
    assert t.phase == "adversarial" and len(hist) == 2 and all(np.isfinite(v) for pair in hist for v in pair)
    mdir = os.path.join(str(root / "a"), "ESRGAN", "model")
    files = os.listdir(mdir)
    assert "ESRGAN_G_param_pretrain.pkl" in files and "ESRGAN_G_param_pretrain_ema.pkl" in files
    assert any(f.startswith("ESRGAN_D_param") for f in files)
    pre = torch.load(os.path.join(mdir, "ESRGAN_G_param_pretrain.pkl"), weights_only=True)
    assert list(pre) == list(t.G.state_dict()) and "body.0.rdb3.conv5.weight" in pre
    assert not torch.equal(pre["conv_first.weight"], t.G.state_dict()["conv_first.weight"].cpu())


@pytest.mark.parametrize("snap", ["snap_pretrain_1.pkl", "snap_adversarial_0.pkl", "snap_adversarial_1.pkl"])
def test_resume_round_trips_in_either_phase(gpu, trained, tmp_path, vgg_file, snap):
    root, extra, t, hist = trained
    want = _final(t)
    path = os.path.join(str(root / "a"), "ESRGAN", snap)
    assert torch.load(path, map_location="cpu", weights_only=True)["phase"] == snap.split("_")[1]
    b, hist_b = _train(_small(_pkg()), _args(tmp_path / "b", 2, vgg_file, "--resume", path, *extra), seed=123)
    got = _final(b)
    assert hist_b == hist and b.phase == "adversarial"
    for k in want:
        assert torch.equal(want[k], got[k]), k


def test_graphed_trainer_matches_eager(gpu, trained, tmp_path, vgg_file):
    """The default (captured) run of the same configuration: the first batch of a shape runs eagerly, the rest replay."""
    root, extra, t, hist = trained
    b, hist_b = _train(_small(_pkg()), _args(tmp_path / "g", 2, vgg_file, *[e for e in extra if e != "--eager"]))
    assert hist_b == hist
    assert torch.equal(b.g_opt.flat.data, t.g_opt.flat.data) and torch.equal(b.d_opt.flat.data, t.d_opt.flat.data)


def test_net_interp_and_test(gpu, trained, vgg_file):
    root, extra, t, hist = trained
    pkg = _pkg()
    Small = _small(pkg)
    x = fill.rand((1, 3, 9, 11), 31)
    mdir = os.path.join(str(root / "a"), "ESRGAN", "model")
    pre = torch.load(os.path.join(mdir, "ESRGAN_G_param_pretrain.pkl"), weights_only=True)
    gan = {k: v.detach().cpu() for k, v in t.G.state_dict().items()}

    def run(*more):
        e = Small(_args(root / "a", 2, vgg_file, "--test_only", *(list(extra) + list(more))))
        return e, e.test_single(x)

    def direct(sd):
        net = pkg.RRDBNet(3, 16, 1, 16, 4)
        net.load_state_dict(sd)
        net.to(gpu).eval()
        with torch.no_grad():
            return net(x.to(gpu)).cpu()

    _, plain = run()
    assert torch.equal(plain, direct(gan))
    assert torch.equal(run("--net_interp", "1")[1], plain)
    assert torch.equal(run("--net_interp", "0")[1], direct(pre)) and not torch.equal(direct(pre), plain)
    e, half = run("--net_interp", "0.5")
    ref = E.RefRRDBNet(3, 16, 1, 16).double()
    ref.load_state_dict({k: 0.5 * pre[k].double() + 0.5 * gan[k].double() for k in gan})
    with torch.no_grad():
        want = ref(x.double())
    assert R.worst(half, want) <= TOL_FWD
    # test() on the blended generator fills PSNR and SSIM
    psnrs = e.test()
    assert len(psnrs) > 0 and all(np.isfinite(psnrs))
    assert e.test_psnr and e.test_ssim and all(np.isfinite(list(e.test_ssim.values())))
    # a missing file is an error that names it
    os.rename(os.path.join(mdir, "ESRGAN_G_param_pretrain.pkl"), os.path.join(mdir, "moved.pkl"))
    try:
        with pytest.raises(FileNotFoundError, match="ESRGAN_G_param_pretrain.pkl"):
            run("--net_interp", "0.5")
    finally:
        os.rename(os.path.join(mdir, "moved.pkl"), os.path.join(mdir, "ESRGAN_G_param_pretrain.pkl"))


def test_trainer_refusals(gpu, tmp_path, vgg_file, monkeypatch):
    import argparse
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    base = vars(_args(tmp_path / "r", 1, vgg_file))
    ns = lambda **kw: argparse.Namespace(**dict(base, **kw))
    for kw, word in ((dict(tile=64), "tile"), (dict(scale_factor=2), "scale_factor"), (dict(net_interp=1.5), "net_interp"),
                     (dict(ssim_weight=0.5), "ssim_weight"), (dict(fft_weight=0.5), "fft_weight"),
                     (dict(lpips_weight=0.5, lpips_vgg="a", lpips_lin="b"), "lpips_weight"), (dict(perceptual=True), "perceptual")):
        with pytest.raises(ValueError, match=word):
            TRAINERS["ESRGAN"](ns(**kw))
    with pytest.raises(ValueError, match="vgg_weights"):
        TRAINERS["ESRGAN"](ns(vgg_weights=None)).train()
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="one GPU"):
        TRAINERS["ESRGAN"](ns())
