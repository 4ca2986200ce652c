"""The JPEG stage on the MI355X: ops.jpeg_u8 byte-equal to the integer restatement in jpeg_ref.py on its case table (the
arithmetic is int32 end to end: no tolerance, nothing left out; tests/test_jpeg_cpu.py holds the restatement to Pillow's
bytes), against Pillow itself, the byte form of the noise, and the loader, the test set and a trainer end to end."""
import functools
import os
import random

import numpy as np
import pytest
import torch

import degrade_ref as R
import jpeg_ref as J

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg(gpu):
    import pytorch_super_resolution_model_collection_amd as p
    return p


@functools.lru_cache(maxsize=None)
def want(name):
    x, q, sub, color = J.case(name)
    return x, q, sub, color, J.jpeg_one(x, q, sub, color)


def dev_jpeg(pkg, gpu, x, quality, sub, color, out_float=False):
    q = quality if isinstance(quality, int) else torch.tensor(quality, dtype=torch.int32, device=gpu)
    y = pkg.ops.jpeg_u8(torch.from_numpy(np.ascontiguousarray(x)).to(gpu), q, subsampling='4:2:0' if sub else '4:4:4',
                        color=bool(color), out_float=out_float)
    assert y.dtype == (torch.float32 if out_float else torch.uint8) and tuple(y.shape) == x.shape
    return y.cpu().numpy()


def mismatch(name, got, ref):
    bad = got != ref
    return "%s: %d of %d bytes differ, first at %s: got %d want %d" % (
        name, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], ref[bad][0]) if bad.any() else ""


@pytest.mark.parametrize("name", J.NAMES)
def test_jpeg_byte_equal_to_restatement(pkg, gpu, name):
    x, q, sub, color, ref = want(name)
    got = dev_jpeg(pkg, gpu, x[None], q, sub, color)[0]
    assert not mismatch(name, got, ref), mismatch(name, got, ref)


def test_jpeg_batch_of_qualities(pkg, gpu):
    """One quality per patch; quality 0 returns its patch, its neighbours do not; out_float is the bytes / 255 in fp32."""
    x, q = J.batch_case()
    assert q == [0, 1, 50, 100, 30]
    for sub in (1, 0):
        ref = J.jpeg(x, q, sub, 1)
        got = dev_jpeg(pkg, gpu, x, q, sub, 1)
        assert not mismatch("batch", got, ref), mismatch("batch", got, ref)
        assert np.array_equal(got[0], x[0]) and all(not np.array_equal(got[b], x[b]) for b in range(1, 5))
        flt = dev_jpeg(pkg, gpu, x, q, sub, 1, out_float=True)
        assert np.array_equal(flt.view(np.uint32), (ref.astype(np.float32) / np.float32(255.0)).view(np.uint32))
    x, q_, sub, color, ref = want([n for n in J.NAMES if "33x31_c1" in n][0])      # fp32 stores that are no whole vector
    flt = dev_jpeg(pkg, gpu, x[None], q_, sub, color, out_float=True)[0]
    assert np.array_equal(flt, ref.astype(np.float32) / np.float32(255.0))
    big = J.content("smooth", 77, (3, 70, 90))[None]                                 # quality 0 across several tiles
    assert np.array_equal(dev_jpeg(pkg, gpu, big, 0, 1, 1), big)
    assert np.array_equal(dev_jpeg(pkg, gpu, big, 0, 1, 1, out_float=True), big.astype(np.float32) / np.float32(255.0))


def test_jpeg_constant_planes_and_argument_errors(pkg, gpu):
    for v in (0, 128, 255):
        for C, color in ((1, 0), (3, 0), (3, 1)):
            p = np.full((2, C, 23, 39), v, np.uint8)
            assert (dev_jpeg(pkg, gpu, p, 75, 1, color) == v).all()
    x = torch.zeros((1, 3, 8, 8), dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError, match="C must be 1 or 3"):
        pkg.ops.jpeg_u8(torch.zeros((1, 2, 8, 8), dtype=torch.uint8, device=gpu), 50, color=False)
    with pytest.raises(RuntimeError, match="color"):
        pkg.ops.jpeg_u8(torch.zeros((1, 1, 8, 8), dtype=torch.uint8, device=gpu), 50, color=True)
    with pytest.raises(ValueError, match="subsampling"):
        pkg.ops.jpeg_u8(x, 50, subsampling='4:2:2')
    with pytest.raises(ValueError, match="0..100"):
        pkg.ops.jpeg_u8(x, 101)
    with pytest.raises(ValueError, match="0..100"):
        pkg.ops.jpeg_u8(x, -1)
    p = torch.from_numpy(J.content("smooth", 3, (3, 17, 9))[None]).to(gpu)      # a tensor's qualities are clamped, as libjpeg's
    assert torch.equal(pkg.ops.jpeg_u8(p, torch.tensor([250], device=gpu)), pkg.ops.jpeg_u8(p, 100))
    assert torch.equal(pkg.ops.jpeg_u8(p, torch.tensor([-4], device=gpu)), pkg.ops.jpeg_u8(p, 1))
    with pytest.raises(RuntimeError, match="integer tensor"):
        pkg.ops.jpeg_u8(x, torch.tensor([50.0], device=gpu))
    with pytest.raises(RuntimeError, match="integer tensor"):
        pkg.ops.jpeg_u8(x, torch.tensor([50, 60], device=gpu))
    with pytest.raises(RuntimeError, match="uint8"):
        pkg.ops.jpeg_u8(x.float(), 50)


@pytest.mark.parametrize("name", ["noise_70x90_c3rgb_s1_", "noise_23x39_c3_s0_"])
def test_jpeg_equals_pillow(pkg, gpu, name):
    if not J.turbo():
        pytest.skip("Pillow is not built on libjpeg-turbo: its bytes are not the ones the definition restates")
    full = [n for n in J.NAMES if n.startswith(name)]
    assert len(full) == 1
    x, q, sub, color = J.case(full[0])
    got, ref = dev_jpeg(pkg, gpu, x[None], q, sub, color)[0], J.pillow_one(x, q, sub, color)
    assert not mismatch(full[0], got, ref), mismatch(full[0], got, ref)


@pytest.mark.parametrize("name", [c[0] for c in R.NOISE_CASES])
def test_noise_bytes_over_255_is_noise(pkg, gpu, name):
    x, sigma, seed = R.noise_case(name)
    xs, sg = torch.from_numpy(x).to(gpu), torch.from_numpy(np.asarray(sigma, np.float64)).to(gpu)
    b = pkg.ops.noise_u8_bytes(xs, sg, seed)
    assert b.dtype == torch.uint8 and b.shape == xs.shape
    f = pkg.ops.noise_u8(xs, sg, seed).cpu().numpy()
    assert np.array_equal((b.cpu().numpy().astype(np.float32) / np.float32(255.0)).view(np.uint32), f.view(np.uint32))
    assert np.array_equal(b.cpu().numpy(), J.noise_bytes(x, sigma, seed))
    assert np.array_equal(f.view(np.uint32), R.noise(x, sigma, seed).view(np.uint32))     # srk_noise_u8 keeps its bits


# -- end to end --------------------------------------------------------------------------------------------------------
def _loader(pkg, gpu, folder, is_gray, jpeg=True):
    kw = dict(R.E2E["degradation"], **(J.E2E_JPEG if jpeg else {}))
    ds = pkg.data.TrainDatasetFromFolder([folder], is_gray=is_gray, crop_size=R.E2E["crop_size"],
                                         scale_factor=R.E2E["scale_factor"], device=gpu, degrade=pkg.data.Degradation(**kw))
    return pkg.data.PatchLoader(ds, R.E2E["batch"], shuffle=False, num_threads=2, background=False)


def _batches(loader):
    random.seed(R.E2E["seed"])
    return [tuple(t.cpu() for t in b) for b in loader]


@pytest.mark.parametrize("is_gray", [False, True])
def test_loader_batches_bit_equal_to_mirror(pkg, gpu, tmp_path, is_gray):
    folder = R.make_folder(str(tmp_path / "train"))
    want_b = J.replay_batches(folder, 2, is_gray)
    got = _batches(_loader(pkg, gpu, folder, is_gray))
    assert len(got) == 2
    for k, ((lr, hr, bc), w) in enumerate(zip(got, want_b)):
        assert lr.shape == (2, 3, 8, 8) and hr.shape == (2, 3, 32, 32) and bc.shape == hr.shape
        assert lr.dtype == hr.dtype == bc.dtype == torch.float32
        for name, a, b in (("lr", lr, w["lr"]), ("hr", hr, w["hr"]), ("bc", bc, w["bc"])):
            assert torch.equal(a, torch.from_numpy(b)), (k, name, float((a - torch.from_numpy(b)).abs().max()))
    plain = _batches(_loader(pkg, gpu, folder, is_gray, jpeg=False))
    assert torch.equal(got[0][1], plain[0][1])                                   # hr is untouched
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(got, plain))          # lr is not
    again = _batches(_loader(pkg, gpu, folder, is_gray))                         # the same seed, the same batches
    for a, b in zip(got, again):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("is_gray,degrade", [(False, None), (False, R.TEST_DEGRADE), (True, R.TEST_DEGRADE)])
def test_test_set_under_jpeg(pkg, gpu, tmp_path, is_gray, degrade):
    from PIL import Image
    from oracle import dataset_pil as O
    folder = R.make_folder(str(tmp_path / "Set5"))
    sf = R.E2E["scale_factor"]
    ds = pkg.data.get_test_set(str(tmp_path), "Set5", sf, is_gray=is_gray, device=gpu, degrade=degrade, jpeg=J.TEST_JPEG)
    clean = O.TestDatasetFromFolder(folder, is_gray=is_gray, scale_factor=sf)
    for i in range(2):
        img = Image.open(ds.image_filenames[i]).convert("RGB")
        hwc = np.asarray(img.convert("YCbCr") if is_gray else img, dtype=np.uint8)
        lr_want = J.item_lr_of_test_set(hwc, sf, degrade, i, J.TEST_JPEG, is_gray)
        lr, hr, bc = (t.cpu() for t in ds[i])
        assert torch.equal(lr, torch.from_numpy(lr_want))
        assert torch.equal(hr, clean[i][1]) and not torch.equal(lr, clean[i][0])
        assert torch.equal(bc, torch.from_numpy(R.bicubic_of_lr(lr_want[None], hr.shape[1], hr.shape[2])[0]))
        lr2, hr2, bc2 = (t.cpu() for t in ds[i])
        assert torch.equal(lr, lr2) and torch.equal(bc, bc2) and torch.equal(hr, hr2)


def test_trainer_trains_and_tests_with_jpeg(pkg, gpu, tmp_path):
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    root = str(tmp_path / "Data")
    R.make_folder(os.path.join(root, "DIV2K", "DIV2K_train_LR_bicubic", "X4"))
    R.make_folder(os.path.join(root, "Set5"), sizes=R.FOLDER_SIZES[:2])
    args = cli.parse_args(["--model_name", "EDSR", "--num_epochs", "1", "--save_epochs", "1", "--batch_size", "2",
                           "--crop_size", "32", "--lr", "1e-4", "--num_threads", "2", "--data_dir", root,
                           "--test_dataset", "Set5", "--save_dir", str(tmp_path / "out"), "--degrade",
                           "--jpeg_quality", "30,95", "--jpeg_test", "40"])
    t = TRAINERS["EDSR"](args)
    hist = t.train()
    assert len(hist) == 1 and np.isfinite(hist).all() and t.data_source == "folder"
    psnr = t.test()
    assert len(psnr) == 2 and np.isfinite(psnr).all() and list(t.test_psnr) == ["Set5"]
