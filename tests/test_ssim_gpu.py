"""SSIM on the device (csrc/ssim.hip: k_ssim_partial / k_ssim_final; ops.ssim, utils.SSIM, test(), main.py --test_only)
against the fp64 numpy restatement of tests/ssim_ref.py, on the case table that tests/test_ssim_cpu.py holds the host twin to.

SSIM_TOL = 1e-6 absolute on every case: tables print four decimals, so it is 50 times under half a printed unit; fp64
accumulation sits orders of magnitude below it; plain fp32 moments miss it on the constant pair by two orders (1.3e-4:
the rounded window does not sum to 1, and E[x^2] - mu^2 turns that into a bias against C2 = 9e-4).  The value leaves the
kernel as fp32, which costs at most 6e-8 of it.  PSNR_RTOL = 1e-5 relative is the bar of test_prepost_gpu's
test_psnr_on_device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import fill, ref_modules as M
import ssim_ref as R

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-6
PSNR_RTOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def laid_out(a, layout, gpu):
    """The fp32 [N,C,H,W] array on the device with the strides of `layout`."""
    t = torch.from_numpy(a).to(gpu)
    if layout == 'nchw':
        return t.contiguous()
    if layout == 'channels_last':
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    big = torch.full((a.shape[0], a.shape[1], a.shape[2] + 5, a.shape[3] + 9), 7.0, device=gpu)
    big[:, :, 2:2 + a.shape[2], 6:6 + a.shape[3]] = t
    return big[:, :, 2:2 + a.shape[2], 6:6 + a.shape[3]]


def check(got, want, what, psnr_too=True):
    s, p, m = [float(v) for v in got]
    print("%-60s ssim %.9f (fp64 %.9f, off by %.2e)  psnr %.6f (fp64 %.6f)" % (what, s, want[0], abs(s - want[0]), p, want[1]))
    assert abs(s - want[0]) <= SSIM_TOL, (what, s, want[0])
    if psnr_too:
        assert abs(p - want[1]) <= PSNR_RTOL * want[1], (what, p, want[1])
        assert abs(m - want[2]) <= 1e-5 * want[2] + 1e-12, (what, m, want[2])


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_ops_ssim_matches_the_restatement(gpu, layout):
    """Every case, domain and crop of the table; prediction in `layout`, target NCHW beside a channels-last prediction."""
    pkg = _pkg()
    for name, p, g, domain, shave in R.combos():
        want = R.ssim_ref(p, g, shave, domain)
        pd, gd = laid_out(p, layout, gpu), laid_out(g, 'nchw' if layout == 'channels_last' else layout, gpu)
        got = pkg.ops.ssim(pd, gd, shave, domain)
        assert all(v.dim() == 0 and v.is_cuda and v.dtype == torch.float32 for v in got)
        check(got, want, "%s %s shave %d %s" % (name, domain, shave, layout))
        if domain == 'float' and shave == 0 and not np.isnan(p).any():
            other = float(pkg.utils.PSNR(pd, gd))
            assert abs(float(got[1]) - other) <= PSNR_RTOL * other, (name, float(got[1]), other)
        if name == "identical":
            assert float(got[1]) == 100.0 and float(got[2]) == 0.0 and abs(float(got[0]) - 1) <= 1e-7
    # [C,H,W] is one image; utils.SSIM is the first output and moves a CPU target over
    p, g = R.cases()["batch_rgb"]
    one = pkg.ops.ssim(torch.from_numpy(p[0]).to(gpu), torch.from_numpy(g[0]).to(gpu), 4, 'y8')
    check(one, R.ssim_ref(p[:1], g[:1], 4, 'y8'), "[C,H,W] y8 shave 4")
    s = pkg.utils.SSIM(torch.from_numpy(p).to(gpu), torch.from_numpy(g), 4, 'u8')
    assert s.dim() == 0 and s.is_cuda and float(s) == float(pkg.ops.ssim(torch.from_numpy(p).to(gpu), torch.from_numpy(g).to(gpu), 4, 'u8')[0])


def test_more_than_four_channels_and_tile_edges(gpu):
    """C > 4 runs one channel per block; sizes around the kernel's 8 x 64 tile of positions (and a 16 x 64 one): exact
    multiples, one over, one under, a single position."""
    pkg = _pkg()
    rng = np.random.RandomState(3)
    for shape in ((1, 6, 40, 90), (2, 1, 26, 74), (1, 3, 27, 75), (1, 2, 25, 73), (1, 4, 42, 138), (1, 1, 11, 11),
                  (1, 3, 18, 74), (1, 1, 19, 139), (2, 2, 17, 137)):
        g = rng.rand(*shape).astype(np.float32)
        p = (g + 0.1 * rng.randn(*shape)).astype(np.float32)
        for domain in ('float', 'u8'):
            check(pkg.ops.ssim(torch.from_numpy(p).to(gpu), torch.from_numpy(g).to(gpu), 0, domain),
                  R.ssim_ref(p, g, 0, domain), "%s %s" % (shape, domain))


def _picture_pair(rng, n, c, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    g = np.stack([0.5 + 0.4 * np.sin(xx / (11.0 + k)) * np.cos(yy / (17.0 + k)) for k in range(n * c)]).reshape(n, c, h, w)
    g = np.clip(g + 0.02 * rng.standard_normal(g.shape).astype(np.float32), 0, 1).astype(np.float32)
    p = (g + 0.04 * rng.standard_normal(g.shape).astype(np.float32)).astype(np.float32)
    return p, g


def test_picture_sized(gpu):
    """3 x 1356 x 2040, the prediction channels-last as a net returns it, the target NCHW as a loader does."""
    pkg = _pkg()
    p, g = _picture_pair(np.random.RandomState(5), 1, 3, 1356, 2040)
    pd = torch.from_numpy(p).to(gpu).contiguous(memory_format=torch.channels_last)
    gd = torch.from_numpy(g).to(gpu)
    for domain, shave in (('float', 0), ('y8', 4), ('u8', 0)):
        check(pkg.ops.ssim(pd, gd, shave, domain), R.ssim_ref(p, g, shave, domain), "picture %s shave %d" % (domain, shave))


def test_element_offsets_beyond_two_to_the_31(gpu):
    """Views whose element offsets pass 2^31: the last image of a batch whose images lie 2^30 elements apart (the index
    arithmetic is 64-bit).  8 GiB of device memory plus 4 GiB for the target; skipped, not shrunk, if that is not there."""
    pkg = _pkg()
    stride_n = 1 << 30
    try:
        store_p = torch.empty(2 * stride_n + (1 << 20), dtype=torch.float32, device=gpu)
        store_g = torch.empty(stride_n + (1 << 20), dtype=torch.float32, device=gpu)
    except RuntimeError as e:   # torch.cuda.OutOfMemoryError is one
        pytest.skip("no room for 12 GiB of device tensors: %s" % (str(e).splitlines()[0],))
    p, g = _picture_pair(np.random.RandomState(6), 3, 3, 60, 200)
    pd = torch.as_strided(store_p, (3, 3, 60, 200), (stride_n, 1, 200 * 3, 3))       # channels-last images, 4 GiB apart
    gd = torch.as_strided(store_g, (3, 3, 60, 200), (stride_n // 2, 60 * 200, 200, 1))
    pd.copy_(torch.from_numpy(p))
    gd.copy_(torch.from_numpy(g))
    assert (pd.shape[0] - 1) * pd.stride(0) >= 2 ** 31
    for domain in ('float', 'y8'):
        check(pkg.ops.ssim(pd, gd, 2, domain), R.ssim_ref(p, g, 2, domain), "offsets past 2^31, %s" % domain)
    del store_p, store_g, pd, gd
    torch.cuda.empty_cache()


def test_two_calls_are_bit_equal_whatever_the_workspace_held(gpu):
    pkg = _pkg()
    lib = pkg._lib.load()
    p, g = _picture_pair(np.random.RandomState(8), 2, 3, 300, 500)
    pd, gd = torch.from_numpy(p).to(gpu).contiguous(memory_format=torch.channels_last), torch.from_numpy(g).to(gpu)
    a = torch.stack(pkg.ops.ssim(pd, gd, 4, 'y8')).cpu()
    b = torch.stack(pkg.ops.ssim(pd, gd, 4, 'y8')).cpu()
    assert torch.equal(a, b)
    from pytorch_super_resolution_model_collection_amd._lib import ptr, stream_ptr
    from pytorch_super_resolution_model_collection_amd.ops import _strides4
    for fill_byte in (0, 0xFF, 0x7F):     # zeros, NaNs, large doubles
        ws = torch.full((int(lib.srk_ssim_workspace_bytes()),), fill_byte, dtype=torch.uint8, device=gpu)
        out = torch.empty(3, device=gpu)
        assert lib.srk_ssim(ptr(pd), _strides4(pd), ptr(gd), _strides4(gd), 2, 3, 300, 500, 4, 2, ptr(out[0:1]), ptr(out[1:2]),
                            ptr(out[2:3]), ptr(ws), stream_ptr()) == 0
        assert torch.equal(out.cpu(), a)
    # the PSNR / MSE outputs are optional
    ws = torch.empty(int(lib.srk_ssim_workspace_bytes()), dtype=torch.uint8, device=gpu)
    out = torch.full((3,), -7.0, device=gpu)
    assert lib.srk_ssim(ptr(pd), _strides4(pd), ptr(gd), _strides4(gd), 2, 3, 300, 500, 4, 2, ptr(out[0:1]), None, None, ptr(ws),
                        stream_ptr()) == 0
    assert out.cpu().tolist() == [float(a[0]), -7.0, -7.0]


def test_ops_ssim_raises_before_launching(gpu):
    pkg = _pkg()
    z = torch.zeros(1, 3, 32, 32, device=gpu)
    with pytest.raises(RuntimeError, match="pred .* vs gt"):
        pkg.ops.ssim(z, torch.zeros(1, 3, 32, 31, device=gpu))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.ops.ssim(z, z.cpu())
    with pytest.raises(RuntimeError, match="10 x 32"):
        pkg.ops.ssim(z[:, :, :10], z[:, :, :10])
    with pytest.raises(RuntimeError, match="under the 11 x 11 window"):
        pkg.ops.ssim(z, z, shave=11)
    with pytest.raises(RuntimeError, match="shave -1"):
        pkg.ops.ssim(z, z, shave=-1)
    with pytest.raises(RuntimeError, match="'y8' takes 1 or 3 channels"):
        pkg.ops.ssim(z[:, :2], z[:, :2], domain='y8')
    with pytest.raises(RuntimeError, match="domain"):
        pkg.ops.ssim(z, z, domain='ycbcr')
    with pytest.raises(RuntimeError, match="expects"):
        pkg.ops.ssim(z[0, 0], z[0, 0])


def test_nothing_waits_for_the_device(gpu):
    pkg = _pkg()
    p, g = R.cases()["batch_rgb"]
    pd, gd = torch.from_numpy(p).to(gpu).contiguous(memory_format=torch.channels_last), torch.from_numpy(g).to(gpu)
    pkg.ops.ssim(pd, gd)     # the library is loaded and the kernel's LDS limit raised
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = pkg.ops.ssim(pd, gd, 4, 'y8')
        b = pkg.utils.SSIM(pd, gd)
        c = pkg.utils.SSIM(pd, gd, 8, 'u8')
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check(a, R.ssim_ref(p, g, 4, 'y8'), "sync debug y8")
    assert abs(float(b) - R.ssim_ref(p, g)[0]) <= SSIM_TOL and abs(float(c) - R.ssim_ref(p, g, 8, 'u8')[0]) <= SSIM_TOL


# ---- test() and main.py ---------------------------------------------------------------------------------------------
SCALE = 4


def _trainer(name, nc, make, tmp, extra=()):
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    args = cli.parse_args(["--model_name", name, "--num_channels", str(nc), "--scale_factor", str(SCALE), "--synthetic",
                           "--save_dir", str(tmp)] + list(extra))
    t = TRAINERS[name](args)
    ora = make().eval()
    t.model = t.build_model()
    t.model.load_state_dict(ora.state_dict())
    t.model.to(t.device).eval()
    return t


def _edsr(tmp, extra=()):
    return _trainer("EDSR", 3, lambda: fill.fill_module(M.EDSR(3, 64, 16), gain=0.5), tmp, extra)


def _loader():
    out = []
    for i in range(3):
        lr = fill.rand((1, 3, 12 + i, 10), 60 + i)
        hr = fill.rand((1, 3, 4 * (12 + i), 40), 70 + i)
        bc = (hr + 0.05 * fill.randn(tuple(hr.shape), 80 + i)).clamp(0, 1)
        out.append((lr, hr, bc))
    return out


def test_test_reports_ssim_beside_psnr(gpu, tmp_path):
    pkg = _pkg()
    loader = _loader()
    t = _edsr(tmp_path / "a")
    psnr = t.test(loader, save_images=True, eval_domain='y8', eval_shave=4)
    outs = [t._infer(lr.to(gpu)) for lr, _, _ in loader]
    # the returned list is what it was: the PSNR kernel on the same tensors, bit for bit
    assert psnr == [float(pkg.utils.PSNR(o, hr.to(gpu))) for o, (_, hr, _) in zip(outs, loader)]
    assert t.test_psnr == {"loader": sum(psnr) / len(psnr)}
    want = [float(pkg.utils.SSIM(o, hr.to(gpu))) for o, (_, hr, _) in zip(outs, loader)]
    assert t.test_ssim == {"loader": sum(want) / len(want)}
    for o, (_, hr, _), w in zip(outs, loader, want):
        assert abs(w - R.ssim_ref(o.cpu().numpy(), hr.numpy())[0]) <= SSIM_TOL
    bc = [float(pkg.utils.SSIM(b.to(gpu), hr.to(gpu))) for _, hr, b in loader]
    assert t.test_bicubic_ssim == {"loader": sum(bc) / len(bc)}
    assert set(t.test_bicubic_psnr) == {"loader"}

    # test_eval: the restatement on the PNGs this very call wrote, against the targets quantised and converted on the host
    rdir = os.path.join(str(tmp_path / "a"), "EDSR", "test_result", "loader")
    ss, ps = [], []
    for i, (_, hr, _) in enumerate(loader):
        y = np.asarray(Image.open(os.path.join(rdir, "SR_result_%d.png" % (i + 1))).convert('YCbCr'))[:, :, 0]
        ty = R.pillow_luma(R.quantise(hr.numpy()))[0, 0]
        y, ty = R.crop(y.astype(np.float64), 4), R.crop(ty.astype(np.float64), 4)
        ss.append(float(R.ssim_map(y, ty, 255.0).mean()))
        ps.append(10 * np.log10(1 / np.mean(((y - ty) / 255.0) ** 2)))
    ev = t.test_eval["loader"]
    print("test_eval %s; from the PNGs: ssim %.9f psnr %.6f" % (ev, np.mean(ss), np.mean(ps)))
    assert ev["domain"] == 'y8' and ev["shave"] == 4
    assert abs(ev["ssim"] - np.mean(ss)) <= SSIM_TOL and abs(ev["psnr"] - np.mean(ps)) <= PSNR_RTOL * np.mean(ps)

    # without the new arguments: the same list, SSIM still reported, no test_eval, no bicubic numbers
    t2 = _edsr(tmp_path / "b")
    assert t2.test(loader) == psnr and t2.test_ssim == t.test_ssim
    assert not hasattr(t2, "test_eval") and not hasattr(t2, "test_bicubic_ssim")
    # args.eval_domain / args.eval_shave are the fall-back; one of the two is enough (shave 0 / domain 'float')
    t3 = _edsr(tmp_path / "c", ["--eval_domain", "u8"])
    assert t3.test(loader) == psnr
    assert t3.test_eval["loader"]["domain"] == 'u8' and t3.test_eval["loader"]["shave"] == 0
    u8 = [R.ssim_ref(o.cpu().numpy(), hr.numpy(), 0, 'u8') for o, (_, hr, _) in zip(outs, loader)]
    assert abs(t3.test_eval["loader"]["ssim"] - np.mean([v[0] for v in u8])) <= SSIM_TOL
    assert abs(t3.test_eval["loader"]["psnr"] - np.mean([v[1] for v in u8])) <= PSNR_RTOL * np.mean([v[1] for v in u8])
    # a pair under the window stays out of the SSIM average and is no error
    small = [(fill.rand((1, 3, 2, 10), 1), fill.rand((1, 3, 8, 40), 2))] + [item[:2] for item in loader]
    t4 = _edsr(tmp_path / "d")
    assert len(t4.test(small)) == 4 and t4.test_ssim == t.test_ssim


def test_cli_test_only_prints_the_numbers_and_never_trains(gpu, tmp_path):
    """main.py --test_only --synthetic in a child process: a PSNR / SSIM line per dataset, and train() never runs."""
    code = ("import sys, runpy\n"
            "sys.argv = ['main.py'] + sys.argv[1:]\n"
            "import pytorch_super_resolution_model_collection_amd.sr_trainers as T\n"
            "def no_train(self, *a, **k):\n"
            "    raise SystemExit('train() was called')\n"
            "for cls in set(T.TRAINERS.values()):\n"
            "    cls.train = no_train\n"
            "runpy.run_path(%r, run_name='__main__')\n" % os.path.join(ROOT, "main.py"))
    argv = ["--model_name", "ESPCN", "--num_channels", "1", "--scale_factor", "4", "--synthetic", "--save_dir", str(tmp_path),
            "--test_only", "--eval_domain", "y8", "--eval_shave", "4"]
    r = subprocess.run([sys.executable, "-c", code] + argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("synthetic: ")]
    assert len(lines) == 1 and "Epoch" not in r.stdout
    import re
    m = re.match(r"synthetic: ESPCN PSNR (\d+\.\d{4}) SSIM (-?\d\.\d{4}), y8 shave 4: PSNR (\d+\.\d{4}) SSIM (-?\d\.\d{4})$", lines[0])
    assert m, lines[0]
    assert all(np.isfinite(float(v)) for v in m.groups()) and abs(float(m.group(2))) <= 1
