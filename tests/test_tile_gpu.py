"""Tiled super-resolution on the GPU: the gather / stitch kernels of csrc/tile.hip against plain indexing and against the
two-launch tail, and test_single(tile=...) / test(tile=...) of every net against the REFERENCE's one-pass output (the
oracle nets on the CPU), not against the product's own one-pass run."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from conftest import rel_err
from oracle import fill, img_interp as O, ref_modules as R

pytestmark = pytest.mark.gpu

SCALE = 4
TOL_FWD = 1e-4   # tests/test_nets_gpu.py: the project's bar for a whole-net forward


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def _tiling():
    from pytorch_super_resolution_model_collection_amd import tiling
    return tiling


# ---- kernels: gather then stitch with no net ------------------------------------------------------------------------
def _layouts(pic, gpu):
    """the same [C,H,W] values behind three kinds of strides"""
    c, h, w = pic.shape
    planar = pic.to(gpu)
    cl = pic.permute(1, 2, 0).contiguous().to(gpu).permute(2, 0, 1)
    big = torch.zeros(c, h + 3, w + 9)
    big[:, 2:2 + h, 5:5 + w] = pic
    strided = big.to(gpu)[:, 2:2 + h, 5:5 + w]
    assert not strided.is_contiguous() and (c == 1 or not cl.is_contiguous())
    return {"planar": planar, "channels_last": cl, "row_strided": strided}


@pytest.mark.parametrize("reach", [0, 5])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw,tile", [((45, 67), 20), ((131, 157), 48), ((33, 16), 16), ((17, 250), 64)])
def test_gather_then_stitch_is_the_identity(gpu, hw, tile, c, reach):
    ops, tiling = _pkg().ops, _tiling()
    h, w = hw
    g = tiling.Geometry(1, 0, -reach, reach)
    plan = tiling.plan(g, h, w, tile)
    tp = ops.TilePlan(plan, gpu)
    pic = fill.randn((c, h, w), 3 + h + c)
    for name, src in _layouts(pic, gpu).items():
        tiles = ops.tile_gather(src, tp)
        assert tuple(tiles.shape) == (plan.ntiles, c, plan.th, plan.tw)
        for t, (y0, x0), _ in plan.tiles():                                       # the gather is plain slicing
            assert torch.equal(tiles[t].cpu(), pic[:, y0:y0 + plan.th, x0:x0 + plan.tw]), (name, t)
        assert torch.equal(ops.tile_stitch(tiles, tp).cpu(), pic), name
        assert torch.equal(ops.tile_stitch(tiles.contiguous(), tp).cpu(), pic), name   # NCHW tile outputs
        # chunked: two tiles at a time, t0 > 0, into one destination that starts as NaN
        out = torch.full((c, h, w), float("nan"), device=gpu)
        for t0 in range(0, plan.ntiles, 2):
            n = min(2, plan.ntiles - t0)
            chunk = ops.tile_gather(src, tp, t0, n)
            assert torch.equal(chunk, tiles[t0:t0 + n])
            ops.tile_stitch(chunk, tp, t0, out)
        assert torch.equal(out.cpu(), pic), name


def _awkward(shape, seed):
    """values below 0, above 1, NaN and exact multiples of 1/255"""
    x = fill.randn(shape, seed) * 0.7 + 0.5
    flat = x.view(-1)
    k = torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=flat.numel() // 3).astype(np.float32))
    flat[: k.numel()] = k / 255
    flat[torch.from_numpy(np.random.RandomState(seed + 1).randint(0, flat.numel(), size=64))] = float("nan")
    return x


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("c", [1, 3])
def test_stitch_u8_is_bit_equal_to_the_two_launch_tail(gpu, c, layout):
    ops, tiling = _pkg().ops, _tiling()
    g = tiling.Geometry(4, 0, -143, 143)                      # EDSR x4
    plan = tiling.plan(g, 131, 157, 96)
    bounds = [o[1] for o in plan.rows.own[:-1]] + [o[1] for o in plan.cols.own[:-1]]
    assert bounds and all(b % 16 for b in bounds)             # ownership boundaries off the 16-pixel grid
    assert plan.OW % 16 and (plan.OW * 3) % 16
    tp = ops.TilePlan(plan, gpu)
    tiles = _awkward((plan.ntiles, c, plan.oth, plan.otw), 40 + c).to(gpu)
    if layout == "channels_last":
        tiles = tiles.contiguous(memory_format=torch.channels_last)
    pic = ops.tile_stitch(tiles, tp)
    assert bool(torch.isnan(pic).any()) and float(pic.nan_to_num().min()) < 0 and float(pic.nan_to_num().max()) > 1
    want = ops.to_u8_image(pic)
    assert torch.equal(ops.tile_stitch_u8(tiles, tp), want)
    out = torch.full_like(want, 77)
    for t0 in range(0, plan.ntiles, 5):                       # chunked
        ops.tile_stitch_u8(tiles[t0:t0 + 5], tp, t0, out)
    assert torch.equal(out, want)
    if c == 1:
        cbcr = torch.from_numpy(np.random.RandomState(9).randint(0, 256, size=(2, plan.OH, plan.OW), dtype=np.uint8)).to(gpu)
        want = ops.ycbcr_to_rgb_u8(pic, cbcr[0], cbcr[1])
        assert torch.equal(ops.tile_stitch_u8(tiles, tp, cb=cbcr[0], cr=cbcr[1]), want)
        out = torch.full_like(want, 77)
        for t0 in range(0, plan.ntiles, 5):
            ops.tile_stitch_u8(tiles[t0:t0 + 5], tp, t0, out, cbcr[0], cbcr[1])
        assert torch.equal(out, want)


def test_tile_ops_reject_what_they_do_not_cover(gpu):
    ops, tiling = _pkg().ops, _tiling()
    plan = tiling.plan(tiling.Geometry(1, 0, -2, 2), 40, 40, 16)
    tp = ops.TilePlan(plan, gpu)
    with pytest.raises(RuntimeError):
        ops.tile_gather(torch.zeros(1, 41, 40, device=gpu), tp)                  # not the plan's picture
    with pytest.raises(RuntimeError):
        ops.tile_gather(torch.zeros(2, 40, 40, device=gpu), tp)                  # C must be 1 or 3
    with pytest.raises(RuntimeError):
        ops.tile_gather(torch.zeros(1, 40, 40), tp)                              # host tensor
    with pytest.raises(RuntimeError):
        ops.tile_gather(torch.zeros(1, 40, 40, device=gpu), tp, plan.ntiles - 1, 2)
    with pytest.raises(RuntimeError):
        ops.tile_stitch(torch.zeros(2, 1, 16, 15, device=gpu), tp)
    with pytest.raises(RuntimeError):
        ops.tile_stitch_u8(torch.zeros(2, 3, 16, 16, device=gpu), tp, cb=torch.zeros(40, 40, dtype=torch.uint8, device=gpu),
                           cr=torch.zeros(40, 40, dtype=torch.uint8, device=gpu))


# ---- nets, against the reference --------------------------------------------------------------------------------------
# name -> (num_channels, oracle net, tile, picture (H, W)).  HR-input nets (SRCNN, VDSR) get the small picture: `tile`
# counts pixels of the net's input.  Every case gives at least 3 x 2 tiles with a shifted last row and column.
BIG, SMALL = (131, 157), (45, 67)
MODELS = {
    "VDSR": (1, lambda: fill.fill_module(R.VDSR(1, 64, 18)), 96, SMALL),
    "ESPCN": (1, lambda: fill.fill_module(R.ESPCN(1, 64, SCALE)), 64, BIG),
    "EDSR": (3, lambda: fill.fill_module(R.EDSR(3, 64, 16), gain=0.5), 96, BIG),          # full depth
    "FSRCNN": (1, lambda: fill.fill_module(R.FSRCNN(1, SCALE, 56, 12, 4)), 64, BIG),
    "SRCNN": (1, lambda: fill.fill_module(R.SRCNN(1, 64)), 64, SMALL),
    "LapSRN": (1, lambda: fill.fill_module(R.LapSRN(1, 64, 10)), 64, BIG),
    "SRGAN": (3, lambda: fill.fill_module(R.Generator(3, 64, 16), gain=0.7), 96, BIG),
}
PATH_MODELS = ("EDSR", "ESPCN", "VDSR")


def _to_tensor(plane_u8):
    """torchvision's ToTensor on an 8-bit array: float32, .div(255)."""
    return torch.from_numpy(np.array(plane_u8, dtype=np.uint8)).float().div(255)


def _trainer(name, tmp):
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    nc, make = MODELS[name][:2]
    args = cli.parse_args(["--model_name", name, "--num_channels", str(nc), "--scale_factor", str(SCALE), "--synthetic",
                           "--save_dir", str(tmp)])
    t = TRAINERS[name](args)
    ora = make().eval()
    t.model = t.build_model()
    t.model.load_state_dict(ora.state_dict())
    t.model.to(t.device).eval()
    return t, ora


def _picture(tmp_path, hw, seed=11, name="picture.png"):
    """A seeded 8-bit picture (odd sizes on purpose): smooth gradients plus noise, so that the nets see image-like input
    and the colour planes are not constant."""
    rs = np.random.RandomState(seed)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([xx / w, yy / h, 0.5 + 0.5 * np.sin(xx / 7.0) * np.cos(yy / 5.0)], axis=-1)
    img = np.clip(base * 255 + rs.normal(0, 20, size=(h, w, 3)), 0, 255).astype(np.uint8)
    fn = str(tmp_path / name)
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


def _oracle_one_pass(name, ora, x):
    with torch.no_grad():
        xin = O.img_interp(x, SCALE, "bicubic") if name in ("VDSR", "SRCNN") else x
        out = ora(xin)
    return out[-1] if isinstance(out, tuple) else out


@pytest.mark.parametrize("name", sorted(MODELS))
def test_single_tiled(gpu, tmp_path, name):
    tiling = _tiling()
    nc, _, tile, hw = MODELS[name]
    t, ora = _trainer(name, tmp_path)
    fn = _picture(tmp_path, hw)
    x, chroma = _reference_input(fn, nc)
    xin = t._net_input(x.to(gpu))
    plan = tiling.plan(tiling.net_geometry(t.model), int(xin.shape[-2]), int(xin.shape[-1]), tile)
    assert len(plan.rows) >= 2 and len(plan.cols) >= 3
    assert plan.rows.starts[-1] == plan.H - plan.th and plan.cols.starts[-1] == plan.W - plan.tw   # shifted inwards
    assert (plan.H - plan.th) % plan.rows.starts[1] and (plan.W - plan.tw) % plan.cols.starts[1]

    # 1. tensor form against the oracle's one-pass output
    want = _oracle_one_pass(name, ora, x)
    got = t.test_single(x, tile=tile)
    assert torch.is_tensor(got) and not got.is_cuda and got.shape == want.shape
    err = rel_err(got, want)
    print("%s tile=%d (%d x %d tiles): tiled vs oracle one pass rel_err %.3e" % (name, tile, len(plan.rows), len(plan.cols), err))
    assert err < TOL_FWD
    for tb in (1, 5, "all"):   # every chunking meets the same bar (not bit-equal: the conv kernels choose by batch size)
        other = t.test_single(x[0], tile=tile, tile_batch=tb)
        print("   tile_batch=%s: rel_err %.3e, against the default chunking %.3e" % (tb, rel_err(other, want), rel_err(other, got)))
        assert rel_err(other, want) < TOL_FWD, tb

    # 4. tile=None returns what it returned before; 'auto' keeps this small picture in one pass
    with torch.no_grad():
        dev_out = t._infer(t._net_input(x.to(gpu)))
    dev_out = (dev_out[-1] if isinstance(dev_out, tuple) else dev_out).cpu()
    assert torch.equal(t.test_single(x), dev_out)
    assert torch.equal(t.test_single(x, tile="auto"), dev_out)
    t.args.tile = tile                                         # the option of the command line
    assert torch.equal(t.test_single(x), got)
    t.args.tile = None
    if name not in PATH_MODELS:
        return

    # 2. path form, exact tail: the reference's Pillow tail on the tiled tensor-form output
    save_fn = t.test_single(fn, tile=tile)
    assert save_fn == os.path.join(str(tmp_path), name, "test_result") + "/SR_result.png"
    png = np.asarray(Image.open(save_fn))
    tail = _reference_tail(got, chroma)
    print("%s exact tail: %d of %d bytes differ" % (name, int((png != tail).sum()), tail.size))
    assert np.array_equal(png, tail)
    tail3 = _reference_tail(t.test_single(x, tile=tile, tile_batch=3), chroma)
    assert np.array_equal(np.asarray(Image.open(t.test_single(fn, tile=tile, tile_batch=3))), tail3)

    # 3. whole chain on the CPU with the oracle: every byte within 1, no share of pixels exempt (the derivation of
    # tests/test_color_gpu.py::test_single_file holds unchanged because step 1 holds)
    chain = _reference_tail(want, chroma)
    diff = np.abs(png.astype(np.int16) - chain.astype(np.int16))
    print("%s whole chain: max byte difference %d, %d of %d bytes differ" % (name, int(diff.max()), int((diff > 0).sum()), diff.size))
    assert png.shape == chain.shape
    assert int(diff.max()) <= 1


def test_drcn_tiled_against_the_stock_composition(gpu, tmp_path):
    """drcn.py:38-52 with torch.nn.functional on the CPU (as tests/test_drcn_gpu.py does) against the tiled trainer."""
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    args = cli.parse_args(["--model_name", "DRCN", "--num_channels", "1", "--scale_factor", str(SCALE), "--synthetic",
                           "--save_dir", str(tmp_path)])
    t = TRAINERS["DRCN"](args)
    t.base_filter, D = 64, t.num_recursions
    t.model = t.build_model()
    fill.fill_module(t.model, seed=11)
    with torch.no_grad():
        t.model.w.copy_(fill.rand((D,), 12, 0.2, 1.0))
    sd = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    w = t.model.w.detach().clone()
    t.model.to(t.device).eval()
    x = fill.rand((1, 1, 17, 20), 13)
    xin = O.img_interp(x, SCALE, "bicubic")

    def conv(h, k, relu):
        y = F.conv2d(h, sd[k + ".conv.weight"], sd[k + ".conv.bias"], padding=1)
        return F.relu(y) if relu else y
    with torch.no_grad():
        h = conv(conv(xin, "embedding_layer.0", True), "embedding_layer.1", True)
        ys = []
        for _ in range(D):
            h = conv(h, "conv_block", True)
            ys.append(conv(conv(h, "reconstruction_layer.0", False), "reconstruction_layer.1", False))
        want = xin + sum(y * w[d] for d, y in enumerate(ys)) / w.sum()
    plan = _tiling().plan(_tiling().net_geometry(t.model), 68, 80, 48)
    assert len(plan.rows) >= 3 and len(plan.cols) >= 3
    got = t.test_single(x, tile=48)
    err = rel_err(got, want)
    print("DRCN tile=48 (%d x %d tiles): rel_err %.3e" % (len(plan.rows), len(plan.cols), err))
    assert err < TOL_FWD


def test_test_with_tiles_reports_the_oracles_psnr_and_writes_the_path_forms_pictures(gpu, tmp_path):
    """Plumbing: test(save_images=True, tile=...) on two seeded pictures.  The PSNR per picture is within 0.01 dB of the
    PSNR computed in fp64 on the CPU from the oracle's one-pass output.  Derived: an output within 1e-4 moves an MSE m by
    at most 2 sqrt(m) 1e-4; for m >= 1e-2 that is under 0.2 % or 0.009 dB (asserted on the oracle side first; an
    untrained net against a random target gives about 0.1)."""
    t, ora = _trainer("EDSR", tmp_path)
    loader, fns, want_db = [], [], []
    for i in range(2):
        fn = _picture(tmp_path, BIG, seed=20 + i, name="p%d.png" % i)
        x, _ = _reference_input(fn, 3)
        hr = fill.rand((1, 3, BIG[0] * SCALE, BIG[1] * SCALE), 30 + i)
        loader.append((x, hr))
        fns.append(fn)
        m = float(((_oracle_one_pass("EDSR", ora, x).double().clamp(0, 1) - hr.double()) ** 2).mean())
        assert m >= 1e-2
        want_db.append(10 * np.log10(1 / m))
    psnr = t.test(loader, save_images=True, tile=96)
    print("tiled test(): PSNR %s, oracle one pass in fp64 %s" % (psnr, want_db))
    assert len(psnr) == 2
    for a, b in zip(psnr, want_db):
        assert abs(a - b) < 0.01
    rdir = os.path.join(str(tmp_path), "EDSR", "test_result", "loader")
    for i, fn in enumerate(fns):
        single = np.asarray(Image.open(t.test_single(fn, tile=96))).copy()
        assert np.array_equal(np.asarray(Image.open(os.path.join(rdir, "SR_result_%d.png" % (i + 1)))), single)


def test_tiled_path_does_not_synchronise(gpu, tmp_path):
    """Between the upload of the picture and the final copy nothing waits for the device -- the upload of the plan's
    table included: with torch's synchronisation debugging set to raise, the tiled forward (fp32 picture) and the tiled
    8-bit tail (chroma resized and merged by the stitch) run through.  One warm call first: the first launch of a net
    packs its filters."""
    ops = _pkg().ops
    t, _ = _trainer("ESPCN", tmp_path)
    rgb = torch.from_numpy(np.array(Image.open(_picture(tmp_path, BIG)))).to(gpu)
    y, cbcr = ops.rgb_to_ycc_planes(rgb, y_float=True)
    x = y.view(1, 1, *BIG)
    want = t._forward(x, 64, 4)
    want8 = t._infer_tiled(x, _tiling().net_geometry(t.model), 64, 4, as_u8=True, chroma=cbcr)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y, cbcr = ops.rgb_to_ycc_planes(rgb, y_float=True)
        x = y.view(1, 1, *BIG)
        size, geo = t._resolve_tile(64, x)
        out = t._forward(x, 64, 4)
        out8 = t._infer_tiled(x, geo, size, 4, as_u8=True, chroma=cbcr)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out, want) and torch.equal(out8, want8)
    assert out8.dtype == torch.uint8 and tuple(out8.shape) == (SCALE * (BIG[0] - 8), SCALE * (BIG[1] - 8), 3)
