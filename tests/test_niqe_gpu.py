"""NIQE on the device (csrc/niqe.hip: k_niqe_scale<1> / <2>; ops.niqe_features, ops.niqe, test(), main.py --niqe_params)
against the numpy / scipy restatement of tests/niqe_ref.py, on the case table and at the bars that tests/test_niqe_cpu.py
holds the host twin to: features |dev - ref| <= 1e-9 max(1, |ref|) with identical NaN positions, the score 1e-6 relative."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import fill, ref_modules as M
import niqe_ref as R

pytestmark = pytest.mark.gpu
SCALE = 4


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


def as_float(u8):
    return (u8.astype(np.float32) / np.float32(255.0)).copy()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_device_matches_the_restatement(gpu, name):
    pkg = _pkg()
    _, _, block, shave, _ = R.CASES[name]
    F, s = R.case_reference(name)
    img = torch.from_numpy(R.case_picture(name).copy()).to(gpu)
    G, gs = pkg.ops.niqe_features(img, shave, block, sharpness=True)
    assert G.dtype == torch.float64 and G.is_cuda and tuple(G.shape) == F.shape and tuple(gs.shape) == s.shape
    R.assert_features(G.cpu().numpy(), F, "device " + name)
    R.assert_features(gs.cpu().numpy(), s, "device " + name + " sharpness")
    only = pkg.ops.niqe_features(img, shave, block)
    assert torch.equal(torch.nan_to_num(only, nan=-7.0), torch.nan_to_num(G, nan=-7.0))


def test_two_calls_and_a_replayed_graph_give_the_same_bits(gpu):
    pkg = _pkg()
    img = torch.from_numpy(as_float(R.case_picture("remainders_nan"))).to(gpu)
    first = pkg.ops.niqe_features(img, 0, 16).clone()
    torch.empty(1 << 20, device=gpu).fill_(float('nan'))       # whatever the next workspace holds does not matter
    second = pkg.ops.niqe_features(img, 0, 16)
    torch.cuda.synchronize()
    assert first.view(torch.int64).equal(second.view(torch.int64))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pkg.ops.niqe_features(img, 0, 16)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pkg.ops.niqe_features(img, 0, 16)
    for _ in range(2):
        out.fill_(0.0)
        graph.replay()
        torch.cuda.synchronize()
        assert out.view(torch.int64).equal(first.view(torch.int64))


def test_every_layout_gives_the_same_bits(gpu):
    pkg = _pkg()
    u8 = torch.from_numpy(R.case_picture("remainders_nan").copy()).to(gpu)
    f = torch.from_numpy(as_float(R.case_picture("remainders_nan"))).to(gpu)
    big = torch.full((3, 57, 83), 0.5, device=gpu)
    big[:, 4:54, 9:79] = f
    tensors = (f.contiguous(), f.permute(1, 2, 0).contiguous().permute(2, 0, 1), big[:, 4:54, 9:79], u8)
    assert tensors[1].stride() == (1, 210, 3) and not tensors[2].is_contiguous()
    outs = [pkg.ops.niqe_features(t, 0, 16).view(torch.int64) for t in tensors]
    for o in outs[1:]:
        assert o.equal(outs[0])
    R.assert_features(outs[0].view(torch.float64).cpu().numpy(), R.case_reference("remainders_nan")[0], "device float NCHW")


def test_score_and_nothing_waits_inside_the_features(gpu):
    pkg = _pkg()
    mu_p, cov_p, rows = R.fitted_params()
    assert np.linalg.cond(cov_p) <= R.COND_MAX
    for name in ("remainders_nan", "grey_block8"):
        _, _, block, shave, _ = R.CASES[name]
        img = torch.from_numpy(R.case_picture(name).copy()).to(gpu)
        pkg.ops.niqe_features(img, shave, block)      # library loaded, tables uploaded, LDS limit raised
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            feats = pkg.ops.niqe_features(img, shave, block)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        want = R.finish(R.case_reference(name)[0], mu_p, cov_p)
        got = pkg.ops.niqe_finish(feats, mu_p, cov_p)
        print("%s: niqe %.9f (restatement %.9f, off by %.2e relative)" % (name, got, want, abs(got - want) / want))
        assert abs(got - want) <= R.SCORE_RTOL * want
        assert pkg.ops.niqe(img, (mu_p, cov_p), shave, block) == got
        assert pkg.utils.NIQE((mu_p, cov_p), shave, block)(img.cpu()) == got
    with pytest.raises(ValueError, match="40 x 31 with 0 pixels shaved from each side holds 1 x 1 blocks of 24 x 24"):
        pkg.ops.niqe_features(torch.zeros(3, 40, 31, device=gpu), 0, 24)


def test_fit_on_the_device_is_the_restatements_fit(gpu):
    pkg = _pkg()
    mu_p, cov_p, rows = R.fitted_params()
    mu, cov, n = pkg.utils.fit_niqe_params([torch.from_numpy(R.picture(100 + i, 3, 64, 80)) for i in range(8)], block=16)
    assert n == rows
    assert np.abs(mu - mu_p).max() <= 1e-9 * max(1.0, np.abs(mu_p).max())
    assert np.abs(cov - cov_p).max() <= 1e-9 * max(1.0, np.abs(cov_p).max())


# ---- test() and main.py ---------------------------------------------------------------------------------------------
def _params_file(tmp):
    mu_p, cov_p, _ = R.fitted_params()
    path = os.path.join(str(tmp), "niqe_params.npz")
    _pkg().utils.save_niqe_params(path, mu_p, cov_p)
    return path


def _edsr(tmp, extra=()):
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    args = cli.parse_args(["--model_name", "EDSR", "--num_channels", "3", "--scale_factor", str(SCALE), "--synthetic",
                           "--save_dir", str(tmp)] + list(extra))
    t = TRAINERS["EDSR"](args)
    ora = fill.fill_module(M.EDSR(3, 64, 16), gain=0.5).eval()
    t.model = t.build_model()
    t.model.load_state_dict(ora.state_dict())
    t.model.to(t.device).eval()
    return t


def _loader():
    out = []
    for i, (h, w) in enumerate(((25, 49), (26, 74))):      # x4, 2 shaved: 96 x 192 (2 blocks), 100 x 292 (3, remainders)
        lr = fill.rand((1, 3, h, w), 160 + i)
        hr = fill.rand((1, 3, 4 * h, 4 * w), 170 + i)
        bc = (hr + 0.05 * fill.randn(tuple(hr.shape), 180 + i)).clamp(0, 1)
        out.append((lr, hr, bc))
    return out


def test_test_reports_niqe_and_leaves_the_rest_alone(gpu, tmp_path):
    pkg = _pkg()
    params = _params_file(tmp_path)
    mu_p, cov_p, _ = R.fitted_params()
    loader = _loader()
    plain = _edsr(tmp_path / "a")
    psnr = plain.test(loader)
    assert not hasattr(plain, "test_niqe") and not hasattr(plain, "test_bicubic_niqe")
    t = _edsr(tmp_path / "b", ["--niqe_params", params, "--eval_shave", "2"])
    assert t.test(loader, save_images=True) == psnr            # PSNR, bit for bit
    assert t.test_psnr == plain.test_psnr and t.test_ssim == plain.test_ssim
    outs = [t._infer(lr.to(gpu)) for lr, _, _ in loader]
    want = [pkg.ops.niqe(o[0], (mu_p, cov_p), 2) for o in outs]
    assert t.test_niqe == {"loader": sum(want) / len(want)}
    bc = [pkg.ops.niqe(b[0].to(gpu), (mu_p, cov_p), 2) for _, _, b in loader]
    assert t.test_bicubic_niqe == {"loader": sum(bc) / len(bc)}
    # the number is the definition's (the host twin: a net's output may hold flat, saturated regions, where only equal
    # window arithmetic agrees on the sign of a zero -- niqe_ref.CASES), of the PNG this very call wrote
    png = np.asarray(Image.open(os.path.join(str(tmp_path / "b"), "EDSR", "test_result", "loader", "SR_result_2.png")))
    ref = pkg.ops.niqe_finish(pkg.ops.niqe_features_host(np.ascontiguousarray(png.transpose(2, 0, 1)), 2, 96), mu_p, cov_p)
    print("test(): niqe of picture 2 %.9f, the host twin on its PNG %.9f" % (want[1], ref))
    assert abs(want[1] - ref) <= R.SCORE_RTOL * ref
    # a picture with fewer than two blocks stays out of the average and is no error
    small = [(fill.rand((1, 3, 12, 10), 1), fill.rand((1, 3, 48, 40), 2))] + [item[:2] for item in loader]
    t2 = _edsr(tmp_path / "c", ["--niqe_params", params, "--eval_shave", "2"])
    assert len(t2.test(small)) == 3 and t2.test_niqe == t.test_niqe and not hasattr(t2, "test_bicubic_niqe")


def test_cli_prints_the_new_field_and_the_old_lines_without_it(gpu, tmp_path, capsys):
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    pkg = _pkg()
    params = _params_file(tmp_path)
    mu_p, cov_p, _ = R.fitted_params()
    base = ["--model_name", "ESPCN", "--num_channels", "1", "--scale_factor", str(SCALE), "--save_dir", str(tmp_path),
            "--crop_size", "232"]                               # synthetic pairs of 58 x 58 -> 200 x 200: 2 x 2 blocks
    t = TRAINERS["ESPCN"](cli.parse_args(base + ["--synthetic"]))
    t.model = t.build_model().to(t.device)
    t.save_model()
    capsys.readouterr()

    cli.main(base + ["--synthetic", "--test_only"])
    old = [l for l in capsys.readouterr().out.splitlines() if l.startswith("synthetic: ")]
    net = cli.main(base + ["--synthetic", "--test_only", "--niqe_params", params])
    new = [l for l in capsys.readouterr().out.splitlines() if l.startswith("synthetic: ")]
    assert len(old) == 1 and len(new) == 1 and " NIQE " not in old[0]
    assert new[0] == old[0] + " NIQE %.4f" % net.test_niqe["synthetic"]
    assert np.isfinite(net.test_niqe["synthetic"])

    fn = os.path.join(str(tmp_path), "in.png")
    Image.fromarray(R.picture(21, 3, 40, 62).transpose(1, 2, 0).copy()).save(fn)    # ESPCN x4: (40 - 8) * 4 = 128 x 216
    cli.main(base + ["--test_single", fn])
    old = capsys.readouterr().out.splitlines()
    cli.main(base + ["--test_single", fn, "--niqe_params", params])
    new = capsys.readouterr().out.splitlines()
    assert not any(l.startswith("NIQE") for l in old)
    assert new[:-1] == old and new[-1].startswith("NIQE ")
    save_fn = os.path.join(str(tmp_path), "ESPCN", "test_result", "SR_result.png")
    assert old[-1] == save_fn
    png = np.ascontiguousarray(np.asarray(Image.open(save_fn)).transpose(2, 0, 1))   # the colour-restored bytes
    want = pkg.ops.niqe_finish(pkg.ops.niqe_features_host(png, 0, 96), mu_p, cov_p)   # the host twin, see test() above
    assert new[-1] == "NIQE %.4f" % pkg.ops.niqe(torch.from_numpy(png).to(gpu), (mu_p, cov_p))
    assert abs(float(new[-1].split()[1]) - want) <= 1e-4 * max(1.0, want)            # four printed decimals


def test_cli_niqe_fit_writes_the_file_and_refuses_to_overwrite(gpu, tmp_path, capsys):
    import main as cli
    pkg = _pkg()
    pics = tmp_path / "pristine"
    pics.mkdir()
    imgs = [R.picture(300 + i, 3, 200, 392) for i in range(6)]      # 2 x 4 blocks of 96 each
    for i, img in enumerate(imgs):
        Image.fromarray(img.transpose(1, 2, 0).copy()).save(str(pics / ("p%d.png" % i)))
    out = str(tmp_path / "fitted.npz")
    argv = ["--save_dir", str(tmp_path), "--niqe_fit", str(pics), "--niqe_params", out]
    cli.main(argv)
    text = capsys.readouterr().out
    mu, cov, rows = pkg.utils.fit_niqe_params([torch.from_numpy(i) for i in imgs])
    assert rows == 48 and ("fitted from %d blocks of 6 pictures" % rows) in text      # all 6 x 8 blocks are sharp enough
    got = pkg.utils.load_niqe_params(out)
    assert np.array_equal(got[0], mu) and np.array_equal(got[1], cov)
    with pytest.raises(SystemExit):
        cli.main(argv)
    assert "does not overwrite" in capsys.readouterr().err
