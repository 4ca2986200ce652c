"""The colour tail on the GPU against Pillow executed now: the three kernels of csrc/color.hip bit-exact on every
24-bit input and on awkward sizes, test_single(path) against the reference's own tail (edsr.py:276-322) and against the
whole CPU chain with the oracle nets, and test(save_images=True)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import fill, img_interp as O, ref_modules as R
pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 17), (3, 5), (339, 510), (37, 100), (16, 128)]   # (H, W)


def every_triple():
    """The 4096 x 4096 x 3 image that holds every 8-bit triple once: pixel i = (i >> 16, (i >> 8) & 255, i & 255)."""
    i = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8)
    return np.ascontiguousarray(img.reshape(4096, 4096, 3))


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _rand_u8(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, size=shape, dtype=np.uint8)


def _to_tensor(plane_u8):
    """torchvision's ToTensor on an 8-bit array: float32, .div(255)."""
    return torch.from_numpy(np.array(plane_u8, dtype=np.uint8)).float().div(255)


def _pil_ycc(rgb):
    return np.asarray(Image.fromarray(np.ascontiguousarray(rgb), "RGB").convert("YCbCr"))


def _pil_rgb(ycc):
    return np.asarray(Image.fromarray(np.ascontiguousarray(ycc), "YCbCr").convert("RGB"))


def _check_rgb_to_ycc(ops, img_dev, img_np):
    ref = _pil_ycc(img_np)
    y, cb, cr = ops.rgb_to_ycbcr_u8(img_dev)
    assert y.dtype == cb.dtype == cr.dtype == torch.uint8 and y.is_cuda
    for got, k, what in ((y, 0, "Y"), (cb, 1, "Cb"), (cr, 2, "Cr")):
        assert np.array_equal(got.cpu().numpy(), ref[:, :, k]), what
    yf, cb2, cr2 = ops.rgb_to_ycbcr_u8(img_dev, y_float=True)
    assert yf.dtype == torch.float32
    assert torch.equal(yf.cpu(), _to_tensor(ref[:, :, 0])), "fp32 Y plane is not ToTensor()(y_plane)"
    assert torch.equal(cb2, cb) and torch.equal(cr2, cr)


# ---- k_rgb_to_ycc ---------------------------------------------------------------------------------------------------
def test_rgb_to_ycbcr_every_rgb_triple(gpu):
    img = every_triple()
    _check_rgb_to_ycc(_pkg().ops, torch.from_numpy(img).to(gpu), img)


@pytest.mark.parametrize("hw", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_rgb_to_ycbcr_awkward_sizes(gpu, hw):
    img = _rand_u8(hw + (3,), 100 + hw[1])
    _check_rgb_to_ycc(_pkg().ops, torch.from_numpy(img).to(gpu), img)


@pytest.mark.parametrize("x0,x1", [(7, 60), (16, 48), (0, 79)])
def test_rgb_to_ycbcr_row_strided_view(gpu, x0, x1):
    base = _rand_u8((20, 80, 3), 5)
    view = torch.from_numpy(base).to(gpu)[:, x0:x1]
    assert not view.is_contiguous()
    _check_rgb_to_ycc(_pkg().ops, view, base[:, x0:x1])


# ---- k_ycc_to_rgb ---------------------------------------------------------------------------------------------------
def _check_ycc_to_rgb(ops, ycc, gpu):
    t = torch.from_numpy(ycc).to(gpu)
    planes = [t[:, :, k].contiguous() for k in range(3)]
    out = ops.ycbcr_to_rgb_u8(*planes)
    assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == ycc.shape
    assert np.array_equal(out.cpu().numpy(), _pil_rgb(ycc))


def test_ycbcr_to_rgb_every_ycc_triple(gpu):
    _check_ycc_to_rgb(_pkg().ops, every_triple(), gpu)


@pytest.mark.parametrize("hw", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_ycbcr_to_rgb_awkward_sizes(gpu, hw):
    _check_ycc_to_rgb(_pkg().ops, _rand_u8(hw + (3,), 200 + hw[1]), gpu)


@pytest.mark.parametrize("hw", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("layout", ["nchw", "channels_last_slice"])
def test_ycbcr_to_rgb_quantises_a_float_y_like_to_pil_image(gpu, hw, layout):
    """The fused form: fp32 Y of any strides -> the bytes of merge(ToPILImage(y.clamp(0, 1)), cb, cr).convert('RGB')."""
    ops = _pkg().ops
    h, w = hw
    y = fill.randn((1, 1, h, w), 31 + w) * 0.6 + 0.5           # values below 0 and above 1 included
    cbcr = _rand_u8((2, h, w), 300 + w)
    if layout == "nchw":
        yd = y.to(gpu)
    else:                                                       # one channel of a 3-channel channels-last buffer
        yd = torch.stack([y[0, 0], y[0, 0] + 1, y[0, 0] - 1], -1).to(gpu)[:, :, 0]
        assert tuple(yd.stride()) == (3 * w, 3)
    y8 = y[0, 0].clamp(0, 1).mul(255).byte().numpy()
    ref = _pil_rgb(np.stack([y8, cbcr[0], cbcr[1]], axis=-1))
    c = torch.from_numpy(cbcr).to(gpu)
    assert np.array_equal(ops.ycbcr_to_rgb_u8(yd, c[0], c[1]).cpu().numpy(), ref)


# ---- k_to_u8 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SIZES + [(45, 67)], ids=["%dx%d" % s for s in SIZES + [(45, 67)]])
@pytest.mark.parametrize("c", [1, 3])
def test_to_u8_image_equals_clamp_mul_byte(gpu, c, hw):
    ops = _pkg().ops
    h, w = hw
    x = fill.randn((1, c, h, w), 41 + w + c) * 0.7 + 0.5        # below 0 and above 1 included
    k = torch.from_numpy(_rand_u8((h * w * c,), 43 + w)[: max(1, h * w * c // 3)].astype(np.float32))
    x.view(-1)[: k.numel()] = k / 255                            # exactly k / 255
    ref = x[0].clamp(0, 1).mul(255).byte().permute(1, 2, 0).numpy()
    for xd in (x.to(gpu), x.to(gpu).contiguous(memory_format=torch.channels_last), x[0].to(gpu)):
        out = ops.to_u8_image(xd)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (h, w, c)
        assert np.array_equal(out.cpu().numpy(), ref), tuple(xd.stride())


@pytest.mark.parametrize("w,x0", [(37, 3), (64, 4), (100, 0)])
def test_float_inputs_as_row_strided_views(gpu, w, x0):
    """A crop along the width of a larger tensor (row stride != width): k_to_u8 and the float-Y form of k_ycc_to_rgb."""
    ops = _pkg().ops
    h = 19
    big = fill.randn((3, h, 120), 51 + w) * 0.7 + 0.5
    view = big.to(gpu)[:, :, x0:x0 + w]
    assert not view.is_contiguous()
    ref = big[:, :, x0:x0 + w].clamp(0, 1).mul(255).byte().permute(1, 2, 0).numpy()
    assert np.array_equal(ops.to_u8_image(view).cpu().numpy(), ref)
    assert np.array_equal(ops.to_u8_image(view[1:2]).cpu().numpy(), ref[:, :, 1:2])
    cbcr = _rand_u8((2, h, w), 53 + w)
    c = torch.from_numpy(cbcr).to(gpu)
    want = _pil_rgb(np.stack([ref[:, :, 0], cbcr[0], cbcr[1]], axis=-1))
    assert np.array_equal(ops.ycbcr_to_rgb_u8(view[0], c[0], c[1]).cpu().numpy(), want)


def test_to_u8_image_nan_gives_zero(gpu):
    ops = _pkg().ops
    x = fill.rand((3, 9, 33), 47)
    ref = x.clamp(0, 1).mul(255).byte().permute(1, 2, 0).numpy().copy()
    x[1, 4, 7] = float("nan")
    x[0, 0, 0] = float("nan")
    x[2, 8, 32] = float("inf")
    x[2, 8, 31] = float("-inf")
    ref[4, 7, 1] = 0
    ref[0, 0, 0] = 0
    ref[8, 32, 2] = 255
    ref[8, 31, 2] = 0
    assert np.array_equal(ops.to_u8_image(x.to(gpu)).cpu().numpy(), ref)


def test_ops_reject_what_they_do_not_cover(gpu):
    ops = _pkg().ops
    with pytest.raises(RuntimeError):
        ops.to_u8_image(torch.zeros(2, 4, 4, device=gpu))                       # C must be 1 or 3
    with pytest.raises(RuntimeError):
        ops.rgb_to_ycbcr_u8(torch.zeros(4, 4, 3, device=gpu))                   # float image
    with pytest.raises(RuntimeError):
        ops.rgb_to_ycbcr_u8(torch.zeros(4, 4, 3, dtype=torch.uint8))            # host tensor: no CPU fallback
    with pytest.raises(RuntimeError):
        ops.ycbcr_to_rgb_u8(torch.zeros(4, 5, dtype=torch.uint8, device=gpu), torch.zeros(4, 4, dtype=torch.uint8, device=gpu),
                            torch.zeros(4, 4, dtype=torch.uint8, device=gpu))


def test_tail_ops_do_not_synchronise(gpu):
    """Between the upload and the final copy the tail must not wait for the device: with torch's synchronisation
    debugging set to raise, the four ops of the tail run through."""
    ops = _pkg().ops
    rgb = torch.from_numpy(_rand_u8((45, 67, 3), 3)).to(gpu)
    y_net = fill.rand((1, 1, 180, 268), 4).to(gpu)
    x3 = fill.rand((1, 3, 45, 67), 5).to(gpu)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y, cbcr = ops.rgb_to_ycc_planes(rgb, y_float=True)
        cbcr = ops.resize_u8(cbcr, 180, 268)
        out = ops.ycbcr_to_rgb_u8(y_net, cbcr[0], cbcr[1])
        out3 = ops.to_u8_image(x3)
        xin = ops.resize_u8(rgb.permute(2, 0, 1), 45, 67, out_float=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(out.shape) == (180, 268, 3) and tuple(out3.shape) == (45, 67, 3)
    assert torch.equal(xin.cpu(), _to_tensor(rgb.cpu().numpy()).permute(2, 0, 1))


# ---- test_single(path) ----------------------------------------------------------------------------------------------
SCALE = 4
MODELS = {  # name -> (num_channels, oracle net)
    "VDSR": (1, lambda: fill.fill_module(R.VDSR(1, 64, 18))),
    "ESPCN": (1, lambda: fill.fill_module(R.ESPCN(1, 64, SCALE))),
    "EDSR": (3, lambda: fill.fill_module(R.EDSR(3, 64, 16), gain=0.5)),
}


def _trainer(name, tmp):
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    nc, make = MODELS[name]
    args = cli.parse_args(["--model_name", name, "--num_channels", str(nc), "--scale_factor", str(SCALE), "--synthetic",
                           "--save_dir", str(tmp)])
    t = TRAINERS[name](args)
    ora = make().eval()
    t.model = t.build_model()
    t.model.load_state_dict(ora.state_dict())
    t.model.to(t.device).eval()
    return t, ora


def _picture(tmp_path):
    """A seeded 8-bit picture, 67 wide and 45 high (odd on purpose): smooth gradients plus noise, so that the nets see
    image-like input and the colour planes are not constant."""
    rs = np.random.RandomState(11)
    h, w = 45, 67
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([xx / w, yy / h, 0.5 + 0.5 * np.sin(xx / 7.0) * np.cos(yy / 5.0)], axis=-1)
    img = np.clip(base * 255 + rs.normal(0, 20, size=(h, w, 3)), 0, 255).astype(np.uint8)
    fn = str(tmp_path / "picture.png")
    Image.fromarray(img, "RGB").save(fn)
    return fn


def _reference_input(fn, nc):
    """edsr.py:289-299: the tensor the reference feeds the net, and the chroma images it keeps."""
    img = Image.open(fn).convert("RGB")
    if nc == 1:
        img_y, img_cb, img_cr = img.convert("YCbCr").split()
        return _to_tensor(np.asarray(img_y)).view(1, 1, img.height, img.width), (img_cb, img_cr)
    return _to_tensor(np.asarray(img)).permute(2, 0, 1).contiguous().view(1, 3, img.height, img.width), None


def _reference_tail(recon, chroma):
    """edsr.py:305-313 on the host: clamp, ToPILImage, bicubic Cb / Cr, merge, convert."""
    recon = recon[0].clamp(0, 1)
    arr = recon.mul(255).byte().permute(1, 2, 0).numpy()                         # ToPILImage
    if chroma is None:
        return np.asarray(Image.fromarray(np.ascontiguousarray(arr), "RGB"))
    recon_y = Image.fromarray(np.ascontiguousarray(arr[:, :, 0]), "L")
    recon_cb = chroma[0].resize(recon_y.size, Image.BICUBIC)
    recon_cr = chroma[1].resize(recon_y.size, Image.BICUBIC)
    return np.asarray(Image.merge("YCbCr", [recon_y, recon_cb, recon_cr]).convert("RGB"))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_single_file(gpu, tmp_path, name):
    t, ora = _trainer(name, tmp_path)
    nc = MODELS[name][0]
    fn = _picture(tmp_path)
    x, chroma = _reference_input(fn, nc)

    # 3a. the tensor form is what it was: the net's output for that tensor, on the host
    with torch.no_grad():
        dev_out = t._infer(t._net_input(x.to(gpu)))
    dev_out = (dev_out[-1] if isinstance(dev_out, tuple) else dev_out).cpu()
    single = t.test_single(x)
    assert torch.is_tensor(single) and not single.is_cuda and torch.equal(single, dev_out)
    assert torch.equal(t.test_single(x[0]), dev_out)

    # 3b. the file is where the reference puts it
    save_fn = t.test_single(fn)
    assert save_fn == os.path.join(str(tmp_path), name, "test_result") + "/SR_result.png"
    assert os.path.exists(save_fn)
    assert t.test_single(tmp_path / "picture.png") == save_fn                    # os.PathLike
    got = np.asarray(Image.open(save_fn))
    assert got.dtype == np.uint8 and got.ndim == 3 and got.shape[2] == 3
    if name == "ESPCN":   # crops a border: the chroma follows the size the net returned
        assert got.shape[:2] == tuple(dev_out.shape[-2:]) and got.shape[:2] != (45 * SCALE, 67 * SCALE)
    else:
        assert got.shape[:2] == (45 * SCALE, 67 * SCALE)

    # 1. exact tail: the reference's Pillow tail on the device net's own output
    want = _reference_tail(dev_out, chroma)
    print("%s exact tail: %d of %d bytes differ" % (name, int((got != want).sum()), want.size))
    assert np.array_equal(got, want)

    # 2. whole chain on the CPU with the oracle net: every byte within 1.  Derived, not measured: the device net agrees
    # with the oracle far inside 1e-4, so the two Y values times 255 differ by much less than 1 and truncation moves the
    # byte by at most 1; the chroma bytes are exact; R, G, B are clip8(y + const), 1-Lipschitz in y (for the RGB model
    # each channel is such a truncation itself).  No share of the pixels is exempt.
    with torch.no_grad():
        xin = O.img_interp(x, SCALE, "bicubic") if name == "VDSR" else x
        ora_out = ora(xin)
    chain = _reference_tail(ora_out, chroma)
    diff = np.abs(got.astype(np.int16) - chain.astype(np.int16))
    print("%s whole chain: max byte difference %d, %d of %d bytes differ; net output max abs difference %.3e"
          % (name, int(diff.max()), int((diff > 0).sum()), diff.size, float((dev_out - ora_out).abs().max())))
    assert got.shape == chain.shape
    assert int(diff.max()) <= 1


def test_cli_test_single_loads_the_checkpoint_and_does_not_train(gpu, tmp_path, capsys):
    import main as cli
    t, _ = _trainer("ESPCN", tmp_path)
    t.save_model()                                    # <save_dir>/ESPCN/model/ESPCN_param.pkl
    fn = _picture(tmp_path)
    want = np.asarray(Image.open(t.test_single(fn))).copy()
    os.remove(os.path.join(str(tmp_path), "ESPCN", "test_result", "SR_result.png"))
    net = cli.main(["--model_name", "ESPCN", "--num_channels", "1", "--scale_factor", str(SCALE), "--save_dir", str(tmp_path),
                    "--test_single", fn])
    out = capsys.readouterr().out
    save_fn = os.path.join(str(tmp_path), "ESPCN", "test_result") + "/SR_result.png"
    assert "Trained model is loaded." in out and save_fn in out and "Epoch" not in out
    assert not hasattr(net, "optimizer")              # train() never ran
    assert np.array_equal(np.asarray(Image.open(save_fn)), want)


# ---- test(loader, save_images=True) ---------------------------------------------------------------------------------
def _loader():
    out = []
    for i in range(3):
        lr = fill.rand((1, 3, 12 + i, 10), 60 + i)
        hr = fill.rand((1, 3, 4 * (12 + i), 40), 70 + i)
        bc = (hr + 0.05 * fill.randn(tuple(hr.shape), 80 + i)).clamp(0, 1)
        out.append((lr, hr, bc))
    return out


def test_test_saves_images_and_reports_the_bicubic_psnr(gpu, tmp_path):
    pkg = _pkg()
    loader = _loader()
    t, _ = _trainer("EDSR", tmp_path / "a")
    psnr = t.test(loader, save_images=True)
    assert len(psnr) == 3 and np.isfinite(psnr).all()
    rdir = os.path.join(str(tmp_path / "a"), "EDSR", "test_result", "loader")
    assert sorted(os.listdir(rdir)) == ["SR_result_1.png", "SR_result_2.png", "SR_result_3.png"]
    bc_vals = []
    for i, (lr, hr, bc) in enumerate(loader):
        out = t._infer(lr.to(gpu)).cpu()
        want = out[0].clamp(0, 1).mul(255).byte().permute(1, 2, 0).numpy()
        assert np.array_equal(np.asarray(Image.open(os.path.join(rdir, "SR_result_%d.png" % (i + 1)))), want)
        bc_vals.append(float(pkg.utils.PSNR(bc.to(gpu), hr.to(gpu))))
    assert set(t.test_bicubic_psnr) == {"loader"}
    assert t.test_bicubic_psnr["loader"] == sum(bc_vals) / len(bc_vals)
    assert t.test_psnr["loader"] == sum(psnr) / len(psnr)

    # without the flag: the same numbers, and no file
    t2, _ = _trainer("EDSR", tmp_path / "b")
    assert t2.test(loader) == psnr
    assert not os.path.exists(os.path.join(str(tmp_path / "b"), "EDSR", "test_result"))
    assert not hasattr(t2, "test_bicubic_psnr")
    # a loader without the bicubic item: images are saved, no baseline is reported
    t3, _ = _trainer("EDSR", tmp_path / "c")
    assert t3.test([item[:2] for item in loader], save_images=True) == psnr
    assert t3.test_bicubic_psnr == {}
    assert len(os.listdir(os.path.join(str(tmp_path / "c"), "EDSR", "test_result", "loader"))) == 3


def test_save_img_one_channel_and_training_name(gpu, tmp_path):
    utils = _pkg().utils
    x = fill.randn((1, 21, 35), 90) * 0.5 + 0.5
    fn = utils.save_img(x.to(gpu), 4, save_dir=str(tmp_path / "r"), is_training=True)
    assert fn == str(tmp_path / "r") + "/SR_result_epoch_4.png"
    got = np.asarray(Image.open(fn))
    assert got.ndim == 2 and np.array_equal(got, x[0].clamp(0, 1).mul(255).byte().numpy())
    fn = utils.save_img(x.expand(3, 21, 35), 5, save_dir=str(tmp_path / "r"))   # a host tensor, as the reference passes
    assert fn.endswith("/SR_result_5.png") and np.asarray(Image.open(fn)).shape == (21, 35, 3)
