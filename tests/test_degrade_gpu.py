"""The training degradations on the MI355X: srk_blur_u8 and srk_noise_u8 byte-equal to the fp64 restatement in
degrade_ref.py on its case table (tests/test_degrade_cpu.py guards that no value of the table rounds within 1e-7 of a
boundary, so nothing is left out and no mismatch is allowed), the identities, the noise's statistics, and the loader, the
test set and a trainer end to end."""
import functools
import os
import random

import numpy as np
import pytest
import torch

import degrade_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg(gpu):
    import pytorch_super_resolution_model_collection_amd as p
    return p


@functools.lru_cache(maxsize=None)
def blur_want(name):
    p, w = R.blur_case(name)
    return p, w, R.blur(p, w)


@functools.lru_cache(maxsize=None)
def noise_want(name):
    x, sigma, seed = R.noise_case(name)
    return x, sigma, seed, R.noise(x, sigma, seed)


def dev_blur(pkg, gpu, p, w):
    y = pkg.ops.blur_u8(torch.from_numpy(p).to(gpu), torch.from_numpy(w).to(gpu))
    assert y.dtype == torch.uint8 and tuple(y.shape) == p.shape
    return y.cpu().numpy()


def dev_noise(pkg, gpu, x, sigma, seed):
    y = pkg.ops.noise_u8(torch.from_numpy(x).to(gpu), torch.from_numpy(np.asarray(sigma, np.float64)).to(gpu), seed)
    assert y.dtype == torch.float32 and tuple(y.shape) == x.shape
    return y.cpu().numpy()


@pytest.mark.parametrize("name", [c[0] for c in R.BLUR_CASES])
def test_blur_byte_equal_to_mirror(pkg, gpu, name):
    p, w, want = blur_want(name)
    got = dev_blur(pkg, gpu, p, w)
    bad = got != want
    assert not bad.any(), "%s: %d of %d bytes differ, first at %s: got %d want %d" % (
        name, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])
    if name == "three_tables":      # the delta among them returns its patch; its neighbours do not
        assert np.array_equal(got[1], p[1]) and not np.array_equal(got[0], p[0]) and not np.array_equal(got[2], p[2])


def test_blur_identities(pkg, gpu):
    p = R.image(41, (2, 3, 37, 29))
    for K in (3, 7, 21):
        assert np.array_equal(dev_blur(pkg, gpu, p, np.stack([R.centred(R.delta(3), K)] * 2)), p)
    w = R.tables(31, 2, 21, ['full'])
    for v in (0, 255):
        assert (dev_blur(pkg, gpu, np.full((2, 1, 24, 24), v, np.uint8), w) == v).all()
    with pytest.raises(RuntimeError, match="K must be odd"):
        pkg.ops.blur_u8(torch.zeros((1, 1, 32, 32), dtype=torch.uint8, device=gpu),
                        torch.zeros((1, 4, 4), dtype=torch.float64, device=gpu))
    with pytest.raises(RuntimeError, match="reflect"):
        pkg.ops.blur_u8(torch.zeros((1, 1, 10, 32), dtype=torch.uint8, device=gpu),
                        torch.zeros((1, 21, 21), dtype=torch.float64, device=gpu))
    with pytest.raises(RuntimeError, match="fp64"):
        pkg.ops.blur_u8(torch.zeros((1, 1, 32, 32), dtype=torch.uint8, device=gpu),
                        torch.zeros((1, 3, 3), dtype=torch.float32, device=gpu))


@pytest.mark.parametrize("name", [c[0] for c in R.NOISE_CASES])
def test_noise_bit_equal_to_mirror(pkg, gpu, name):
    x, sigma, seed, want = noise_want(name)
    got = dev_noise(pkg, gpu, x, sigma, seed)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d of %d values differ" % (name, int(bad.sum()), bad.size)
    for b in np.flatnonzero(sigma == 0):      # sigma 0: x / 255 in fp32, exactly
        assert np.array_equal(got[b], x[b].astype(np.float32) / np.float32(255.0))
    assert sigma.max() == 0 or not np.array_equal(got, x.astype(np.float32) / np.float32(255.0))


def test_noise_extremes_and_statistics(pkg, gpu):
    shape, n = (16, 3, 32, 32), 16 * 3 * 32 * 32
    for v in (0, 255):
        x = np.full(shape, v, np.uint8)
        got = dev_noise(pkg, gpu, x, np.full(16, 25.0), R.STAT_SEED)
        assert got.min() >= 0.0 and got.max() <= 1.0 and np.array_equal(got, R.noise(x, np.full(16, 25.0), R.STAT_SEED))
        assert 0.4 < (got == v / 255.0).mean() < 0.6      # half of the draws push outwards and are clamped
    # constant 128, sigma 10: the range ends 12.8 sigma away, nothing is clamped
    x = np.full(shape, 128, np.uint8)
    d = dev_noise(pkg, gpu, x, np.full(16, 10.0), R.STAT_SEED).astype(np.float64) * 255.0 - 128.0
    print("noise statistics: mean %.5f (bound %.5f), std / 10 - 1 = %.5f (bound 0.02)"
          % (d.mean(), 5 * 10 / np.sqrt(n), d.std() / 10 - 1))
    assert abs(d.mean()) < 5 * 10 / np.sqrt(n)
    # five standard errors 1 / sqrt(2 n) of the estimate = 0.016, plus the 0.4 % that rounding to whole levels adds
    assert abs(d.std() / 10 - 1) < 0.02
    assert np.abs(d - np.round(d)).max() < 1e-4           # whole levels


# -- end to end --------------------------------------------------------------------------------------------------------
def _loader(pkg, gpu, folder, is_gray, degrade=True):
    deg = pkg.data.Degradation(**R.E2E["degradation"]) if degrade else None
    ds = pkg.data.TrainDatasetFromFolder([folder], is_gray=is_gray, crop_size=R.E2E["crop_size"],
                                         scale_factor=R.E2E["scale_factor"], device=gpu, degrade=deg)
    return ds, pkg.data.PatchLoader(ds, R.E2E["batch"], shuffle=False, num_threads=2, background=False)


def _batches(loader):
    random.seed(R.E2E["seed"])
    return [tuple(t.cpu() for t in b) for b in loader]


@pytest.mark.parametrize("is_gray", [False, True])
def test_loader_batches_bit_equal_to_mirror(pkg, gpu, tmp_path, is_gray):
    folder = R.make_folder(str(tmp_path / "train"))
    want = R.replay_batches(folder, 2, is_gray)
    got = _batches(_loader(pkg, gpu, folder, is_gray)[1])
    assert len(got) == 2
    for k, ((lr, hr, bc), w) in enumerate(zip(got, want)):
        assert lr.shape == (2, 3, 8, 8) and hr.shape == (2, 3, 32, 32) and bc.shape == hr.shape
        assert lr.dtype == hr.dtype == bc.dtype == torch.float32
        for name, a, b in (("lr", lr, w["lr"]), ("hr", hr, w["hr"]), ("bc", bc, w["bc"])):
            assert torch.equal(a, torch.from_numpy(b)), (k, name, float((a - torch.from_numpy(b)).abs().max()))
    clean = _batches(_loader(pkg, gpu, folder, is_gray, degrade=False)[1])
    assert torch.equal(got[0][1], clean[0][1])                      # hr is untouched
    assert not torch.equal(got[0][0], clean[0][0]) and not torch.equal(got[0][2], clean[0][2])   # lr and bc are not
    again = _batches(_loader(pkg, gpu, folder, is_gray)[1])         # the same seed, the same batches
    for a, b in zip(got, again):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_restored_random_state_reproduces_the_next_batch(pkg, gpu, tmp_path):
    """What --resume relies on: every draw of the degradation comes from Python's `random`, whose state the training-state
    file holds.  The state taken after batch 1 of an epoch, restored in another run, gives batch 2."""
    folder = R.make_folder(str(tmp_path / "train"))
    ds, loader = _loader(pkg, gpu, folder, False)
    random.seed(R.E2E["seed"])
    gen = loader._produce()
    next(gen)
    state = random.getstate()
    second = [t.cpu() for t in ds.dev.hand_over(*next(gen)[0])]
    ds2, loader2 = _loader(pkg, gpu, folder, False)
    random.seed(999)
    gen2 = loader2._produce()
    next(gen2)
    random.setstate(state)
    again = [t.cpu() for t in ds2.dev.hand_over(*next(gen2)[0])]
    assert all(torch.equal(a, b) for a, b in zip(second, again))
    random.seed(999)            # ... and it is the state that does it
    ds3, loader3 = _loader(pkg, gpu, folder, False)
    gen3 = loader3._produce()
    next(gen3)
    other = [t.cpu() for t in ds3.dev.hand_over(*next(gen3)[0])]
    assert not torch.equal(other[0], second[0])


@pytest.mark.parametrize("is_gray", [False, True])
def test_test_set_under_a_fixed_degradation(pkg, gpu, tmp_path, is_gray):
    from PIL import Image
    from oracle import dataset_pil as O
    folder = R.make_folder(str(tmp_path / "Set5"))
    sf = R.E2E["scale_factor"]
    ds = pkg.data.get_test_set(str(tmp_path), "Set5", sf, is_gray=is_gray, device=gpu, degrade=R.TEST_DEGRADE)
    clean = O.TestDatasetFromFolder(folder, is_gray=is_gray, scale_factor=sf)
    for i in range(2):
        img = Image.open(ds.image_filenames[i]).convert("RGB")
        hwc = np.asarray(img.convert("YCbCr") if is_gray else img, dtype=np.uint8)
        lr_want = R.item_lr_of_test_set(hwc, sf, R.TEST_DEGRADE, i)
        lr, hr, bc = (t.cpu() for t in ds[i])
        assert torch.equal(lr, torch.from_numpy(lr_want))
        assert torch.equal(hr, clean[i][1]) and not torch.equal(lr, clean[i][0])
        assert torch.equal(bc, torch.from_numpy(R.bicubic_of_lr(lr_want[None], hr.shape[1], hr.shape[2])[0]))
        lr2, hr2, bc2 = (t.cpu() for t in ds[i])      # a second read: the noise is seeded by the index
        assert torch.equal(lr, lr2) and torch.equal(bc, bc2) and torch.equal(hr, hr2)


def test_trainer_trains_and_tests_with_degrade(pkg, gpu, tmp_path):
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    root = str(tmp_path / "Data")
    R.make_folder(os.path.join(root, "DIV2K", "DIV2K_train_LR_bicubic", "X4"))
    R.make_folder(os.path.join(root, "Set5"), sizes=R.FOLDER_SIZES[:2])
    args = cli.parse_args(["--model_name", "EDSR", "--num_epochs", "1", "--save_epochs", "1", "--batch_size", "2",
                           "--crop_size", "32", "--lr", "1e-4", "--num_threads", "2", "--data_dir", root,
                           "--test_dataset", "Set5", "--save_dir", str(tmp_path / "out"), "--degrade",
                           "--blur_sigma", "0.4,3.5", "--noise_sigma", "1,12", "--degrade_test", "1.2,2.0,30,5"])
    t = TRAINERS["EDSR"](args)
    hist = t.train()
    assert len(hist) == 1 and np.isfinite(hist).all() and t.data_source == "folder"
    assert os.path.exists(t._ckpt_name(None))
    psnr = t.test()
    assert len(psnr) == 2 and np.isfinite(psnr).all() and list(t.test_psnr) == ["Set5"]
