"""Real-ESRGAN's second-order degradation on the MI355X: srk_noise2_u8, srk_usm_u8, the BOX filter of the
Pillow-exact resampler and signed tables through srk_blur_u8, each byte-equal to its restatement (degrade2_ref.py, Pillow)
with no pixel left out -- tests/test_degrade2_cpu.py guards that no case rounds within 1e-7 of a boundary -- then the whole
chain through the loader, resume, the test sets and two trainers."""
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

import degrade_ref as R1
import degrade2_ref as R
import perceptual_ref as P

pytestmark = pytest.mark.gpu
VGG_SEED = 78


@pytest.fixture(scope="module")
def pkg(gpu):
    import pytorch_super_resolution_model_collection_amd as p
    return p


@pytest.fixture(scope="module")
def cdf(pkg, gpu):
    host = pkg.ops.poisson_cdf()
    return host, torch.from_numpy(host).to(gpu)


def f64(gpu, a):
    return torch.from_numpy(np.asarray(a, np.float64)).to(gpu)


def same_bytes(got, want, what):
    bad = got != want
    assert not bad.any(), "%s: %d of %d bytes differ, first at %s: got %d want %d" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


# -- the kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.NOISE2_CASES])
def test_noise2_byte_equal_to_mirror(pkg, gpu, cdf, name):
    x, mode, gray, amount, seed, stage, color = R.noise2_case(name)
    want = R.noise2(x, mode, gray, amount, cdf[0], seed, stage, color)
    call = lambda: pkg.ops.noise2_u8(torch.from_numpy(x).to(gpu), f64(gpu, mode), f64(gpu, gray), f64(gpu, amount), cdf[1],
                                     seed, stage, color).cpu().numpy()
    got = call()
    same_bytes(got, want, name)
    assert np.array_equal(call(), got)                                   # two calls, the same bytes
    off = mode == 0
    assert np.array_equal(got[off], x[off])                              # mode off returns the patch
    if not off.all():
        assert not np.array_equal(got[~off], x[~off])


def test_noise2_colour_gauss_is_noise_u8_bytes(pkg, gpu, cdf):
    x, sigma, seed = R1.noise_case("three_sigmas")
    B = x.shape[0]
    got = pkg.ops.noise2_u8(torch.from_numpy(x).to(gpu), f64(gpu, np.ones(B)), f64(gpu, np.zeros(B)), f64(gpu, sigma), cdf[1],
                            seed, 0)
    assert torch.equal(got, pkg.ops.noise_u8_bytes(torch.from_numpy(x).to(gpu), f64(gpu, sigma), seed))


@pytest.mark.parametrize("name", [c[0] for c in R.USM_CASES])
def test_usm_byte_equal_to_mirror(pkg, gpu, name):
    x, g, weight, threshold = R.usm_case(name)
    want = R.usm(x, g, weight, threshold)
    gd = f64(gpu, pkg.ops.usm_table(len(g)))
    got = pkg.ops.usm_u8(torch.from_numpy(x).to(gpu), gd, weight, threshold).cpu().numpy()
    same_bytes(got, want, name)
    assert np.array_equal(pkg.ops.usm_u8(torch.from_numpy(x).to(gpu), gd, weight, threshold).cpu().numpy(), got)
    assert np.array_equal(pkg.ops.usm_u8(torch.from_numpy(x).to(gpu), gd, weight, 255.0).cpu().numpy(), x)


def test_usm_defaults_and_constant_plane(pkg, gpu):
    flat = torch.full((2, 3, 30, 41), 137, dtype=torch.uint8, device=gpu)
    assert torch.equal(pkg.ops.usm_u8(flat), flat)
    x, g, weight, threshold = R.usm_case("y_64")
    assert np.array_equal(pkg.ops.usm_u8(torch.from_numpy(x).to(gpu)).cpu().numpy(), R.usm(x, g, weight, threshold))
    with pytest.raises(RuntimeError, match="K / 2"):
        pkg.ops.usm_u8(torch.zeros((1, 3, 25, 40), dtype=torch.uint8, device=gpu))


@pytest.mark.parametrize("case", R.BOX_CASES, ids=lambda c: "%dx%d-to-%dx%d" % (c[1][1], c[1][2], c[2][0], c[2][1]))
def test_box_resize_byte_equal_to_pillow(pkg, gpu, case):
    iseed, shape, (oh, ow) = case
    x = R1.image(iseed, (1,) + shape)[0]
    got = pkg.ops.resize_u8(torch.from_numpy(x).to(gpu), oh, ow, interpolation="box").cpu().numpy()
    same_bytes(got, R.pil_resize(x, oh, ow, R.BOX), "box %s -> %s" % (shape, (oh, ow)))


@pytest.mark.parametrize("table", R.BLUR2_TABLES, ids=lambda t: "%s-K%d" % (t[0], t[1]))
@pytest.mark.parametrize("iseed,shape", R.BLUR2_SHAPES)
def test_signed_and_plateau_tables_through_blur(pkg, gpu, iseed, shape, table):
    """The existing srk_blur_u8, unchanged, under sinc (negative entries: the clamp at both ends works) and plateau tables."""
    p = R1.image(iseed, shape)
    w = np.stack([pkg.ops.blur_table(*table)] * shape[0])
    got = pkg.ops.blur_u8(torch.from_numpy(p).to(gpu), torch.from_numpy(w).to(gpu)).cpu().numpy()
    same_bytes(got, R1.blur(p, np.stack([R.blur_table(*table)] * shape[0])), "%s %s" % (shape, table[:2]))


# -- the chain through the loader -----------------------------------------------------------------------------------------
def _loader(pkg, gpu, folder, is_gray, usm=False):
    ds = pkg.data.TrainDatasetFromFolder([folder], is_gray=is_gray, crop_size=R.E2E["crop_size"],
                                         scale_factor=R.E2E["scale_factor"], device=gpu, usm=usm,
                                         degrade=pkg.data.Degradation2(**R.E2E["overrides"]))
    return ds, pkg.data.PatchLoader(ds, R.E2E["batch"], shuffle=False, num_threads=2, background=False)


@functools.lru_cache(maxsize=None)
def _want(folder, seed, is_gray, usm):
    return R.replay_batch(folder, seed, is_gray=is_gray, usm_on=usm)


@pytest.mark.parametrize("usm", [False, True])
@pytest.mark.parametrize("is_gray", [False, True])
def test_loader_batches_bit_equal_to_mirror(pkg, gpu, tmp_path_factory, is_gray, usm):
    folder = R.make_folder(str(tmp_path_factory.mktemp("d2") / "train"))
    ds, loader = _loader(pkg, gpu, folder, is_gray, usm)
    crop, lr_sz, B = R.E2E["crop_size"], R.E2E["crop_size"] // R.E2E["scale_factor"], R.E2E["batch"]
    drawn = []
    for seed in R.E2E_SEEDS:
        w = _want(folder, seed, is_gray, usm)
        drawn.append(w["p"])
        random.seed(seed)
        lr, hr, bc = (t.cpu() for t in next(iter(loader)))
        assert lr.shape == (B, 3, lr_sz, lr_sz) and hr.shape == (B, 3, crop, crop) and bc.shape == hr.shape
        assert lr.dtype == hr.dtype == bc.dtype == torch.float32
        for name, a, b in (("lr", lr, w["lr"]), ("hr", hr, w["hr"]), ("bc", bc, w["bc"])):
            bad = a != torch.from_numpy(b)
            assert not bool(bad.any()), (seed, name, int(bad.sum()), float((a - torch.from_numpy(b)).abs().max()))
    assert R.coverage(drawn) >= R.WANTED, sorted(R.WANTED - R.coverage(drawn))


def test_restored_random_state_reproduces_the_next_batch(pkg, gpu, tmp_path):
    """What --resume relies on: every draw of the chain comes from Python's `random`, whose state the training-state file
    holds, and nothing else is kept between batches."""
    folder = R.make_folder(str(tmp_path / "train"))
    ds, loader = _loader(pkg, gpu, folder, False, usm=True)
    random.seed(21)
    gen = loader._produce()
    state = random.getstate()
    first = [t.cpu() for t in ds.dev.hand_over(*next(gen)[0])]
    ds2, loader2 = _loader(pkg, gpu, folder, False, usm=True)
    random.seed(999)
    random.setstate(state)
    again = [t.cpu() for t in ds2.dev.hand_over(*next(loader2._produce())[0])]
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    random.seed(999)
    ds3, loader3 = _loader(pkg, gpu, folder, False, usm=True)
    other = [t.cpu() for t in ds3.dev.hand_over(*next(loader3._produce())[0])]
    assert not torch.equal(other[0], first[0])


@pytest.mark.parametrize("is_gray", [False, True])
def test_test_set_items_are_fixed_and_equal_the_mirror(pkg, gpu, tmp_path, is_gray):
    from PIL import Image
    R.make_folder(str(tmp_path / "Set5"))
    sf = R.E2E["scale_factor"]
    d = pkg.data.Degradation2(**R.E2E["overrides"])
    ds = pkg.data.get_test_set(str(tmp_path), "Set5", sf, is_gray=is_gray, device=gpu, degrade2=(d, R.TEST_SEED))
    before = random.getstate()
    for i in range(2):
        img = Image.open(ds.image_filenames[i]).convert("RGB")
        hwc = np.asarray(img.convert("YCbCr") if is_gray else img, dtype=np.uint8)
        want = R.test_item(hwc, sf, R.TEST_SEED, i, is_gray=is_gray)[0]
        lr, hr, bc = (t.cpu() for t in ds[i])
        assert torch.equal(lr, torch.from_numpy(want))
        assert torch.equal(bc, torch.from_numpy(R1.bicubic_of_lr(want[None], hr.shape[1], hr.shape[2])[0]))
        lr2, hr2, bc2 = (t.cpu() for t in ds[i])
        assert torch.equal(lr, lr2) and torch.equal(bc, bc2) and torch.equal(hr, hr2)
    assert random.getstate() == before                   # the items' generators are private
    with pytest.raises(ValueError, match="degrade2"):
        pkg.data.get_test_set(str(tmp_path), "Set5", sf, device=gpu, degrade2=(d, 1), jpeg=40)


# -- the trainers ---------------------------------------------------------------------------------------------------------
def _data(tmp_path):
    root = str(tmp_path / "Data")
    R.make_folder(os.path.join(root, "DIV2K", "DIV2K_train_LR_bicubic", "X4"))
    R1.make_folder(os.path.join(root, "Set5"), sizes=R.FOLDER_SIZES[:2])
    settings = str(tmp_path / "degrade2.json")
    with open(settings, "w") as f:
        json.dump({"resize_range": [0.5, 1.5]}, f)
    return root, settings


def _state(t):
    mods = [m for m in (getattr(t, "model", None), getattr(t, "G", None), getattr(t, "D", None)) if m is not None]
    return [v.detach().clone() for m in mods for v in m.state_dict().values()]


def _run(cls, args, seed=0):
    torch.manual_seed(seed)
    random.seed(seed)
    t = cls(args)
    hist = t.train()
    torch.cuda.synchronize()
    return t, hist


def test_edsr_trains_tests_and_resumes_with_degrade2_and_usm(pkg, gpu, tmp_path):
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    root, settings = _data(tmp_path)

    def args(save, epochs, *extra):
        return cli.parse_args(["--model_name", "EDSR", "--num_epochs", str(epochs), "--save_epochs", "1", "--batch_size", "2",
                               "--crop_size", "48", "--lr", "1e-4", "--num_threads", "2", "--data_dir", root, "--eager",
                               "--test_dataset", "Set5", "--save_dir", str(tmp_path / save), "--degrade2", settings, "--usm",
                               "--degrade2_test", "5"] + list(extra))
    a, hist_a = _run(TRAINERS["EDSR"], args("a", 2))
    assert len(hist_a) == 2 and np.isfinite(hist_a).all() and a.data_source == "folder"
    assert os.path.exists(a._ckpt_name(None))
    psnr = a.test()
    assert len(psnr) == 2 and np.isfinite(psnr).all()
    b1, hist_b1 = _run(TRAINERS["EDSR"], args("b", 1))
    b2, hist_b2 = _run(TRAINERS["EDSR"], args("b", 2, "--resume"), seed=123)
    assert hist_b1 == hist_a[:1] and hist_b2 == hist_a
    for x, y in zip(_state(a), _state(b2)):
        assert torch.equal(x, y)


def test_esrgan_unet_trains_with_degrade2_and_usm(pkg, gpu, tmp_path):
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    root, settings = _data(tmp_path)
    vgg = str(tmp_path / "vgg19_head34.pth")
    torch.save(P.filled_head(34, VGG_SEED)[2], vgg)

    class Small(TRAINERS["ESRGAN"]):
        def build_model(self):
            self.G = pkg.RRDBNet(self.num_channels, 16, self.blocks, self.growth, self.scale_factor)
            self.D = self.build_discriminator()
            return self.G

    args = cli.parse_args(["--model_name", "ESRGAN", "--rrdb_blocks", "1", "--rrdb_growth", "16", "--crop_size", "48",
                           "--num_epochs", "2", "--batch_size", "2", "--lr", "1e-3", "--num_threads", "2", "--data_dir", root,
                           "--test_dataset", "Set5", "--save_dir", str(tmp_path / "out"), "--vgg_weights", vgg, "--eager",
                           "--epoch_pretrain", "1", "--save_epochs", "1", "--discriminator", "unet", "--unet_feat", "8",
                           "--degrade2", settings, "--usm"])
    t, hist = _run(Small, args)
    assert isinstance(t.D, pkg.UNetDiscriminatorSN) and t.phase == "adversarial" and t.data_source == "folder"
    assert len(hist) == 2 and all(np.isfinite(v) for pair in hist for v in pair)
    files = os.listdir(os.path.join(str(tmp_path / "out"), "ESRGAN", "model"))
    assert "ESRGAN_G_param_pretrain.pkl" in files and any(f.startswith("ESRGAN_D_param") for f in files)
