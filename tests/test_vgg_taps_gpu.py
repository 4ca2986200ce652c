"""The multi-layer VGG feature loss on the GPU (csrc/vgg_tap.hip, ops.vgg_feature_loss, --vgg_layers): the tap kernels
against the float64 yardstick of tests/vgg_taps_ref.py over the operator table in every mode and input kind, with every
buffer pre-filled with NaN and through pointers one element off a 16-byte boundary; a shape taken from the launcher's own
plan at which a block walks more than one chunk; the seed contract three ways; eager against replayed bits; the whole term
and its composition from the older operators against the fp64 head; and ESRGAN steps that train on the term.

Bars (vgg_taps_ref.py): maps bit-equal, loss within 1e-4 relative, da within 1e-3 * max|ref|; the whole term under
perceptual_ref.bar; the trainer step under the bars of tests/test_esrgan_gpu.py (losses within 5e-4; per parameter tensor
the L2 norm within 5e-4 of it and the sum within 10 * 5e-4 of the norm)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import esrgan_ref as E
import perceptual_ref as P
import vgg_taps_ref as R
from conftest import rel_err
from oracle import fill

pytestmark = pytest.mark.gpu

TOL_STEP = 5e-4
VGG_SEED = 78


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _offset_copy(t, gpu, off):
    """The NCHW CPU tensor t as a dense NHWC device view `off` elements behind a fresh allocation."""
    flat = torch.empty(t.numel() + 1, device=gpu)
    v = flat[off:off + t.numel()].view(t.shape[0], t.shape[2], t.shape[3], t.shape[1])
    v.copy_(t.permute(0, 2, 3, 1))
    return v


def _nan_view(shape, gpu, off):
    """(flat, view): a NaN-filled allocation with one spare element either side of an NHWC view of NCHW `shape`."""
    n, c, h, w = shape
    numel = n * c * h * w
    flat = torch.full((numel + 2,), float("nan"), device=gpu)
    return flat, flat[off:off + numel].view(n, h, w, c)


def _untouched_outside(flat, numel, off):
    return bool(torch.isnan(flat[off + numel:]).all()) and (off == 0 or bool(torch.isnan(flat[0])))


def _run_raw(pkg, case, gpu, off, factor=None):
    """One tap through the C ABI on NaN-filled buffers: (loss, ya, yb, da) as CPU NCHW tensors, after the checks that
    every element was written and nothing outside was."""
    lib = pkg._lib.load()
    mode, shape = case["mode"], tuple(case["a"].shape)
    n, c, h, w = shape
    a, b = _offset_copy(case["a"], gpu, off), _offset_copy(case["b"], gpu, off)
    assert a.data_ptr() % 16 == 4 * off
    ws = torch.full((lib.srk_vgg_tap_workspace_bytes(1) // 8,), float("nan"), dtype=torch.float64, device=gpu)
    loss = torch.full((), float("nan"), device=gpu)
    ya = yb = g = None
    if mode != R.LAST:
        oshape = R.out_shape(shape, mode)
        (fa, ya), (fb, yb) = _nan_view(oshape, gpu, off), _nan_view(oshape, gpu, off)
        g = _offset_copy(case["g"], gpu, off)
    check = pkg._lib.check
    check(lib.srk_vgg_tap_forward(_ptr(a), _ptr(b), n, h, w, c, mode, case["weight"], 0, 1, _ptr(ws), _ptr(ya), _ptr(yb),
                                  None), "srk_vgg_tap_forward")
    check(lib.srk_vgg_tap_finish(_ptr(ws), 1, _ptr(loss), None), "srk_vgg_tap_finish")
    fd, da = _nan_view(shape, gpu, off)
    f = None if factor is None else torch.full((), factor, device=gpu)
    check(lib.srk_vgg_tap_backward(_ptr(a), _ptr(b), _ptr(g), n, h, w, c, mode, case["c"], _ptr(f), _ptr(da), None),
          "srk_vgg_tap_backward")
    torch.cuda.synchronize()
    assert not torch.isnan(ws).any() and not torch.isnan(loss)
    assert not torch.isnan(da).any() and _untouched_outside(fd, da.numel(), off), (shape, off)
    if mode != R.LAST:
        assert not torch.isnan(ya).any() and not torch.isnan(yb).any(), (shape, off)
        assert _untouched_outside(fa, ya.numel(), off) and _untouched_outside(fb, yb.numel(), off), (shape, off)
        ya, yb = R.nchw(ya).cpu(), R.nchw(yb).cpu()
    return float(loss), ya, yb, R.nchw(da).cpu()


def _check_case(pkg, case, gpu, tag):
    for off in (0, 1):     # 16-byte path where C % 4 == 0, then the 4-byte path through misaligned pointers
        loss, ya, yb, da = _run_raw(pkg, case, gpu, off)
        err, scale = P.max_err(da, case["da"])
        print("vgg tap %s off %d: loss %.9g ref %.9g (rel %.2e)  da err %.2e of max |ref| %.2e"
              % (tag, off, loss, case["loss"], abs(loss - case["loss"]) / max(abs(case["loss"]), 1e-300), err, scale))
        assert abs(loss - case["loss"]) <= R.LOSS_CONTRACT * abs(case["loss"])
        assert err <= R.GRAD_CONTRACT * scale
        if case["mode"] != R.LAST:
            assert torch.equal(ya, case["ya"]) and torch.equal(yb, case["yb"])


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape, mode", R.op_cases(), ids=_id)
def test_tap_matches_the_yardstick(gpu, shape, mode, kind):
    _check_case(_pkg(), R.tap_case(shape, mode, kind), gpu, "%s %s %s" % (_id(shape), mode, kind))


@pytest.mark.parametrize("mode", list(R.MODES))
def test_blocks_that_walk_several_chunks(gpu, mode):
    """The smallest plane of 64 channels at which the launcher's plan gives a block of the 16-byte POOL path a second
    chunk; the other modes and the 4-byte path walk several chunks there as well."""
    pkg = _pkg()
    lib = pkg._lib.load()
    shape = R.multi_chunk_shape(lib)
    for vec in (1, 0):
        blocks, items, passes = R.plan_of(lib, shape, R.MODES[mode], vec)
        print("plan %s %s vec %d: %d blocks, %d items, %d passes" % (_id(shape), mode, vec, blocks, items, passes))
        assert passes >= 2
    _check_case(pkg, R.tap_case(shape, mode, "continuous"), gpu, "%s %s continuous" % (_id(shape), mode))


def test_foreign_factor_and_zero_weight(gpu):
    """The device factor multiplies c alone, not the gradient routed from behind the tap; c = 0 leaves that gradient."""
    pkg = _pkg()
    case = R.tap_case((2, 8, 6, 10), "pool", "continuous")
    want3 = R.tap_case((2, 8, 6, 10), "pool", "continuous", seed_value=3.0)["da"]
    _, _, _, da = _run_raw(pkg, case, gpu, 0, factor=3.0)
    err, scale = P.max_err(da, want3)
    assert err <= R.GRAD_CONTRACT * scale
    x = case["a"].double().requires_grad_(True)
    (R.behind(x, R.POOL) * case["g"].double()).sum().backward()
    _, _, _, da0 = _run_raw(pkg, dict(case, c=0.0), gpu, 0)
    assert torch.equal(da0.double(), x.grad)


# ---- the term ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def extractor(gpu):
    pkg = _pkg()
    return pkg.FeatureExtractor(feature_layer=34).load_vgg19(P.filled_head(34)[2]).to(gpu)


def _loss_and_grad(pkg, fe, pred, target, backward):
    p = pred.detach().clone().requires_grad_(True)
    loss = pkg.ops.vgg_feature_loss(p, target, fe, dict(R.REALESRGAN))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    backward(loss)
    return float(loss.detach()), p.grad.detach()


def test_equal_inputs_give_exact_zeros(gpu, extractor):
    pkg = _pkg()
    x = R.term_case(R.TERM_SHAPES[0])["pred"].to(gpu)
    loss, grad = _loss_and_grad(pkg, extractor, x, x.clone(), pkg.ops.backward)
    assert loss == 0.0 and float(grad.abs().max()) == 0.0
    p = x.clone().requires_grad_(True)
    loss = pkg.ops.vgg_feature_loss(p, p, extractor, dict(R.REALESRGAN))     # the very same tensor
    pkg.ops.backward(loss)
    assert float(loss) == 0.0 and float(p.grad.abs().max()) == 0.0


def test_seed_contract_three_ways(gpu, extractor):
    """The unit seed, a seed declared through ops.loss_seed, and a foreign upstream gradient: the same gradient times its
    factor, each against the fp64 head; and the module face and weighted_term / loss_sum on the term."""
    pkg = _pkg()
    ops = pkg.ops
    case = R.term_case(R.TERM_SHAPES[0])
    pred, target = case["pred"].to(gpu), case["target"].to(gpu)
    l_bar = P.bar(R.LOSS_CONTRACT, case["l_err32"], abs(case["l64"]))
    g_bar = P.bar(R.GRAD_CONTRACT, case["d_err32"], float(case["d64"].abs().max()))
    seed = torch.full((), 0.25, device=gpu)

    def declared(loss):
        ops.backward(loss, seed=seed)

    def run_declared():
        p = pred.detach().clone().requires_grad_(True)
        with ops.loss_seed(0.25, seed):
            loss = ops.vgg_feature_loss(p, target, extractor, dict(R.REALESRGAN))
        declared(loss)
        return float(loss.detach()), p.grad.detach()

    runs = {"unit": (_loss_and_grad(pkg, extractor, pred, target, ops.backward), 1.0),
            "declared": (run_declared(), 0.25),
            "foreign": (_loss_and_grad(pkg, extractor, pred, target, lambda l: (2.5 * l).backward()), 2.5)}
    for name, ((loss, grad), factor) in runs.items():
        err = P.max_err(grad, factor * case["d64"])[0]
        print("seed %-8s loss %.9g (fp64 %.9g) grad err %.3e, bar %.3e" % (name, loss, case["l64"], err, factor * g_bar))
        assert abs(loss - case["l64"]) <= l_bar and err <= factor * g_bar
    # the nn.Module face, and the term under weighted_term / loss_sum (the weight declared as its seed)
    mod = pkg.utils.VGGFeatureLoss(dict(R.REALESRGAN), extractor)
    assert float(mod(pred, target)) == runs["unit"][0][0]
    p = pred.detach().clone().requires_grad_(True)
    term = ops.weighted_term(lambda a, b: ops.vgg_feature_loss(a, b, extractor, dict(R.REALESRGAN)), 0.5, p, target)
    ops.backward(ops.loss_sum(ops.l1_loss(p.detach(), target), term, 1.0, 0.5))
    assert P.max_err(p.grad, 0.5 * case["d64"])[0] <= 0.5 * g_bar


def test_eager_calls_and_a_replayed_graph_give_the_same_bits(gpu, extractor):
    pkg = _pkg()
    case = R.term_case(R.TERM_SHAPES[0])
    pred, target = case["pred"].to(gpu), case["target"].to(gpu)

    def fn(p, t):
        p = p.detach().requires_grad_(True)
        loss = pkg.ops.vgg_feature_loss(p, t, extractor, dict(R.REALESRGAN))
        grad, = torch.autograd.grad(loss, p, pkg.ops.unit_seed(p.device))
        return loss, grad

    first = [v.detach().clone() for v in fn(pred, target)]
    second = [v.detach().clone() for v in fn(pred, target)]
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    graph = pkg.trainers.capture_step(fn, (pred, target), warmup=1)
    for _ in range(2):
        out = [v.detach().clone() for v in graph(pred, target)]
        torch.cuda.synchronize()
        assert torch.equal(first[0], out[0]) and torch.equal(first[1], out[1])
    graph.close()


@pytest.mark.parametrize("shape", R.TERM_SHAPES, ids=_id)
def test_term_and_its_composition_match_the_fp64_head(gpu, extractor, shape):
    """The fused term and the same term from the older operators (un-fused conv, ReLU, ops.l1_loss, ops.fork,
    ops.max_pool2x2_train) both land within the same bars of the float64 head: the same function, not merely a close one."""
    pkg = _pkg()
    case = R.term_case(shape)
    pred, target = case["pred"].to(gpu), case["target"].to(gpu)
    l_bar = P.bar(R.LOSS_CONTRACT, case["l_err32"], abs(case["l64"]))
    g_bar = P.bar(R.GRAD_CONTRACT, case["d_err32"], float(case["d64"].abs().max()))
    fused = _loss_and_grad(pkg, extractor, pred, target, pkg.ops.backward)
    p = pred.detach().clone().requires_grad_(True)
    loss = R.composition(pkg, extractor, p, target)
    pkg.ops.backward(loss)
    composed = (float(loss.detach()), p.grad.detach())
    for name, (l, g) in (("fused", fused), ("composition", composed)):
        err = P.max_err(g, case["d64"])[0]
        print("vgg term %s %-11s loss %.9g fp64 %.9g |diff| %.3e (torch fp32 %.3e, bar %.3e)  grad err %.3e of max |ref| "
              "%.3e (torch fp32 %.3e, bar %.3e)" % (_id(shape), name, l, case["l64"], abs(l - case["l64"]), case["l_err32"],
                                                    l_bar, err, float(case["d64"].abs().max()), case["d_err32"], g_bar))
        assert abs(l - case["l64"]) <= l_bar and err <= g_bar


# ---- trainer steps ---------------------------------------------------------------------------------------------------------
def _nets(pkg, gpu, nf=64, nb=1, gc=32, bf=64):
    G, D = pkg.RRDBNet(3, nf, nb, gc, 4), pkg.ESRGANDiscriminator(3, bf, 32)
    fill.fill_module(G, 5, 0.7)
    fill.fill_module(D, 6, 1.0)
    return G.to(gpu).train(), D.to(gpu).train()


def _check_params(net, oracle, tag):
    sd = net.state_dict()
    for n, p in oracle.state_dict().items():
        if not p.is_floating_point():
            continue
        want, t = p.detach().double(), sd[n].detach().double().cpu()
        l2 = float(want.pow(2).sum().sqrt())
        assert abs(float(t.pow(2).sum().sqrt()) - l2) <= TOL_STEP * max(l2, 1e-8), "%s L2 %s" % (tag, n)
        assert abs(float(t.sum()) - float(want.sum())) <= 10 * TOL_STEP * max(l2, 1e-8), "%s sum %s" % (tag, n)


def test_step_matches_the_cpu_oracle(gpu):
    """One adversarial step at nb = 1, batch 2, 8 x 8 LR, 32 x 32 HR with vgg_layers = realesrgan against the fp32 CPU
    oracle step (esrgan_ref's, with the term of vgg_taps_ref.term in the place of the single tap)."""
    pkg = _pkg()
    G, D = _nets(pkg, gpu)
    oG = E.RefRRDBNet(3, 64, 1, 32)
    oG.load_state_dict({k: v.detach().cpu() for k, v in G.state_dict().items()})
    oD = E.ref_discriminator(3, 64, 32)
    oD.load_state_dict({k: v.detach().cpu() for k, v in D.state_dict().items()})
    oG.train()
    oD.train()
    lr_img, hr_img = fill.rand((2, 3, 8, 8), 121), fill.rand((2, 3, 32, 32), 131)
    g_opt = pkg.optim.make_optimizer("esrgan_g", pkg.optim.FlatParams(G), 1e-4)
    d_opt = pkg.optim.make_optimizer("esrgan_d", pkg.optim.FlatParams(D), 1e-4)
    og_opt = torch.optim.Adam(oG.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    od_opt = torch.optim.Adam(oD.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    fe = pkg.FeatureExtractor(feature_layer=34).load_vgg19(P.filled_head(34, VGG_SEED)[2]).to(gpu)
    step = pkg.trainers.esrgan_step(G, D, g_opt, d_opt, fe, vgg_layers=dict(R.REALESRGAN))
    d_loss, g_loss = (float(v.detach()) for v in step(lr_img.to(gpu), hr_img.to(gpu)))
    od, og = R.oracle_adversarial_step(oG, oD, og_opt, od_opt, P.filled_head(34, VGG_SEED)[0], lr_img, hr_img)
    print("vgg_layers step d_loss %.8f oracle %.8f  g_loss %.8f oracle %.8f" % (d_loss, od, g_loss, og))
    assert rel_err(np.array([d_loss, g_loss]), np.array([od, og])) < TOL_STEP
    _check_params(G, oG, "adversarial G")
    _check_params(D, oD, "adversarial D")
    assert all(p.requires_grad for p in D.parameters()) and all(p.grad is None for p in fe.parameters())


def test_default_step_is_the_single_tap_step_bit_for_bit(gpu):
    """vgg_layers=None: esrgan_step against the step restated here around the plain ops.perceptual_loss closure, as it
    was before the flag existed: the same losses and parameters, bit for bit, over two steps."""
    pkg = _pkg()
    ops, T = pkg.ops, pkg.trainers
    batches = [(fill.rand((2, 3, 8, 8), 52 + i).to(gpu), fill.rand((2, 3, 32, 32), 62 + i).to(gpu)) for i in range(2)]
    fe = pkg.FeatureExtractor(feature_layer=34).load_vgg19(P.filled_head(34, VGG_SEED)[2]).to(gpu)

    def plain_step(G, D, g_opt, d_opt, pixel_weight=1e-2, vgg_weight=1.0, gan_weight=5e-3):
        out = {}

        def percep(pred, target):
            return ops.perceptual_loss(pred, target, fe, normalize=True, criterion='l1')

        def seg_g(lr_img, hr_img):
            g_opt.zero_grad()
            fake = G(lr_img)
            f_gan, rest = ops.fork(fake)
            f_pix, f_vgg = ops.fork(rest)
            out["fake"] = fake.detach()
            for p in D.parameters():
                p.requires_grad_(False)
            try:
                real_logits = D(hr_img).detach()
                l_gan = ops.weighted_term(lambda f, r: ops.ragan_loss(r, f, True), gan_weight, D(f_gan), real_logits)
            finally:
                for p in D.parameters():
                    p.requires_grad_(True)
            l_pix = ops.weighted_term(ops.l1_loss, pixel_weight, f_pix, hr_img)
            l_vgg = ops.weighted_term(percep, vgg_weight, f_vgg, hr_img)
            g_loss = ops.loss_sum(ops.loss_sum(l_pix, l_vgg, pixel_weight, vgg_weight), l_gan, 1.0, gan_weight)
            T._backward(g_loss, None)
            g_opt.step()
            out["g"] = g_loss
            return g_loss

        def seg_d(lr_img, hr_img):
            d_opt.zero_grad()
            d_loss = ops.ragan_loss(D(hr_img), D(out.pop("fake")), False)
            T._backward(d_loss, None)
            d_opt.step()
            return d_loss, out.pop("g")

        return T.eager_step([(seg_g, None), (seg_d, None)])

    def run(make_step):
        G, D = _nets(pkg, gpu, 32, 1, 16, 8)
        g_flat, d_flat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
        g_opt = pkg.optim.make_optimizer("esrgan_g", g_flat, 1e-3)
        d_opt = pkg.optim.make_optimizer("esrgan_d", d_flat, 1e-3)
        step = make_step(G, D, g_opt, d_opt)
        losses = [[float(v.detach()) for v in step(*b)] for b in batches]
        return losses, [g_flat.data.clone(), d_flat.data.clone(), g_opt.exp_avg.clone(), d_opt.exp_avg_sq.clone()]

    losses_a, state_a = run(lambda G, D, g_opt, d_opt: T.esrgan_step(G, D, g_opt, d_opt, fe, vgg_layers=None))
    losses_b, state_b = run(plain_step)
    assert losses_a == losses_b
    for i, (a, b) in enumerate(zip(state_a, state_b)):
        assert torch.equal(a, b), i


@pytest.fixture(scope="module")
def vgg_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vgg") / "vgg19_head34.pth")
    torch.save(P.filled_head(34, VGG_SEED)[2], path)
    return path


def _args(save_dir, vgg_file, *extra):
    import main as cli
    return cli.parse_args(["--model_name", "ESRGAN", "--rrdb_blocks", "1", "--rrdb_growth", "16", "--crop_size", "32",
                           "--num_epochs", "2", "--batch_size", "2", "--synthetic", "--steps_per_epoch", "2", "--lr", "1e-3",
                           "--save_dir", str(save_dir), "--vgg_weights", vgg_file, "--vgg_layers", "realesrgan",
                           "--epoch_pretrain", "1", "--save_epochs", "1", "--ema_decay", "0.9"] + list(extra))


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


def test_trainer_eager_replayed_and_resumed_are_bit_equal(gpu, tmp_path, vgg_file):
    """main.py's ESRGAN trainer with --vgg_layers realesrgan: one pre-training epoch and two adversarial ones, run eagerly,
    from captured graphs, and resumed after the first adversarial epoch: the same histories and final states."""
    pkg = _pkg()
    a, hist = _train(_small(pkg), _args(tmp_path / "a", vgg_file, "--eager"))
    assert a.phase == "adversarial" and len(hist) >= 1 and all(np.isfinite(v) for pair in hist for v in pair)
    assert [n for n, _, _ in a.vgg_layers] == [n for n, _ in R.REALESRGAN]
    want = _final(a)
    g, hist_g = _train(_small(pkg), _args(tmp_path / "g", vgg_file))
    assert hist_g == hist
    got = _final(g)
    for k in want:
        assert torch.equal(want[k], got[k]), ("graph", k)
    snap = os.path.join(str(tmp_path / "a"), "ESRGAN", "snap_adversarial_1.pkl")
    b, hist_b = _train(_small(pkg), _args(tmp_path / "b", vgg_file, "--eager", "--resume", snap), seed=123)
    assert hist_b == hist
    got = _final(b)
    for k in want:
        assert torch.equal(want[k], got[k]), ("resume", k)


def test_trainer_with_the_unet_discriminator(gpu, tmp_path, vgg_file):
    """--discriminator unet --gan_type vanilla --vgg_layers (a spec of its own, a RELU-mode tap among them), captured:
    both phases run, the losses are finite and the extractor stops at the deepest named layer."""
    pkg = _pkg()
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS

    class SmallUNet(TRAINERS["ESRGAN"]):
        def build_model(self):
            self.G = pkg.RRDBNet(self.num_channels, 16, self.blocks, self.growth, self.scale_factor)
            self.D = pkg.UNetDiscriminatorSN(self.num_channels, 8)
            return self.G

    args = _args(tmp_path / "u", vgg_file, "--discriminator", "unet", "--gan_type", "vanilla")
    args.vgg_layers = "conv1_2:0.1,conv2_1:0.5,conv3_4:1"
    t, hist = _train(SmallUNet, args)
    assert t.phase == "adversarial" and len(hist) >= 1 and all(np.isfinite(v) for pair in hist for v in pair)
    assert [(n, i) for n, i, _ in t.vgg_layers] == [("conv1_2", 2), ("conv2_1", 5), ("conv3_4", 16)]
