"""LPIPS without a GPU: srk_lpips_layer_host (the kernels' per-pixel bodies, csrc/lpips_common.h, in plain C++ double)
against the fp64 restatement of tests/lpips_ref.py over the layer table, central differences, the argument checks of every
entry point, the weight loading of models.LPIPS, and the refusals of the trainer and CLI arguments.  The device kernels
are held to the same table in tests/test_lpips_gpu.py."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__
import lpips_ref as R

# both sides are fp64 on the same fp32 inputs: only the summation order and 1 / a against a division differ
HOST_TOL = 1e-12


@pytest.fixture(scope="module")
def pkg():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    return p


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


@pytest.mark.parametrize("shape", R.LAYER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_twin_matches_restatement(lib, shape):
    case = R.layer_case(shape)
    value, df0 = R.host_layer(lib, case["f0"], case["f1"], case["w"], case["g"])
    for what, got, want in (("value", value, case["value"]), ("df0", df0, case["df0"])):
        err, scale = R.max_err(got, want)
        print("srk_lpips_layer_host %-12s %-5s max err %.3g of max |ref| %.3g" % (shape, what, err, scale))
        assert err <= HOST_TOL * max(scale, 1e-300), (shape, what, err, scale)
    assert bool(torch.isfinite(df0).all())
    only, _ = R.host_layer(lib, case["f0"], case["f1"], case["w"])
    assert torch.equal(only, value)                       # forward only: the same values


def test_all_zero_pixels_follow_the_vector_norm_rule(lib):
    """f0 = 0 at a pixel: the gradient there is 2 w q / a with q = -f1 / b (the second term is 0 by definition); f1 = 0
    too: a zero gradient; and plain sqrt(sum(f^2)) autograd, which the definition declines, gives NaN there."""
    case = R.layer_case((2, 3, 5, 3))
    _, df0 = R.host_layer(lib, case["f0"], case["f1"], case["w"], case["g"])
    f0, f1 = case["f0"], case["f1"]
    assert float(f0[0, :, 0, 0].abs().max()) == 0.0 and float(f1[0, :, 0, 0].abs().max()) > 0.0
    b = float(torch.linalg.vector_norm(f1[0, :, 0, 0].double())) + R.EPS
    want = float(case["g"][0]) / 15.0 * 2.0 * case["w"].double() * (-f1[0, :, 0, 0].double() / b) / R.EPS
    assert float((df0[0, :, 0, 0] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float(f0[1, :, 2, 4].abs().max()) == 0.0 and float(f1[1, :, 2, 4].abs().max()) == 0.0
    assert float(df0[1, :, 2, 4].abs().max()) == 0.0
    x = f0.double().requires_grad_(True)
    (x / (x.pow(2).sum(1, keepdim=True).sqrt() + R.EPS)).sum().backward()
    assert bool(torch.isnan(x.grad).any())


def test_central_differences(lib):
    f0, f1 = torch.relu(R.fill.randn((1, 5, 2, 3), 981)) + 0.05, torch.relu(R.fill.randn((1, 5, 2, 3), 982))
    w, g = R.fill.rand((5,), 983), torch.tensor([0.7], dtype=torch.float64)
    _, df0 = R.host_layer(lib, f0, f1, w, g)
    # h is exact in fp32 next to values of order 1.  A central difference misses the derivative by h^2 / 6 * d''', and d is
    # a rational function of f0 / ||f0|| with ||f0|| >= 0.05 * sqrt(5) here, so d''' is at most a few hundred: h = 2^-13
    # keeps that below 1e-6; the fp64 values contribute 1e-16 / h = 1e-12.  The bar is 1e-5 of the largest gradient.
    h = 2.0 ** -13
    for idx in [(0, 0, 0, 0), (0, 3, 1, 2), (0, 4, 0, 1), (0, 2, 1, 0)]:
        up, dn = f0.clone(), f0.clone()
        up[idx] += h
        dn[idx] -= h
        fd = float(g[0]) * (float(R.host_layer(lib, up, f1, w)[0][0]) - float(R.host_layer(lib, dn, f1, w)[0][0])) \
            / (float(up[idx]) - float(dn[idx]))
        assert abs(fd - float(df0[idx])) <= 1e-5 * float(df0.abs().max()), (idx, fd, float(df0[idx]))


def test_equal_maps_give_exact_zeros(lib):
    f = torch.relu(R.fill.randn((2, 70, 5, 7), 984))
    value, df0 = R.host_layer(lib, f, f, R.fill.rand((70,), 985), torch.ones(2, dtype=torch.float64))
    assert float(value.abs().max()) == 0.0 and float(df0.abs().max()) == 0.0


def test_planner(lib):
    """One block a sample for the small maps, several for (1, 9, 8, 64); the workspace holds either path's partials."""
    for n, h, w, c in R.LAYER_SHAPES:
        blocks = [lib.srk_lpips_layer_blocks(n, h, w, c, 0)] + ([lib.srk_lpips_layer_blocks(n, h, w, c, 1)] if c % 4 == 0 else [])
        assert min(blocks) >= 1 and lib.srk_lpips_layer_workspace(n, h, w, c) >= 8 * n * max(blocks)
    assert lib.srk_lpips_layer_blocks(1, 9, 8, 64, 1) > 1 and lib.srk_lpips_layer_blocks(1, 4, 4, 64, 1) == 1
    assert lib.srk_lpips_layer_blocks(1, 4000, 4000, 64, 1) == lib.srk_lpips_layer_blocks(1, 8000, 8000, 64, 1)   # capped
    assert lib.srk_lpips_layer_blocks(1, 4, 4, 70, 1) == -1 and b"C % 4" in lib.srk_last_error_string()


def test_argument_checks(lib):
    buf = np.zeros(1 << 12, np.float64)
    p = ctypes.c_void_p(buf.ctypes.data)
    err = lambda: lib.srk_last_error_string()

    def fwd(f0=p, f1=p, w=p, table=p, ws=p, n=2, h=4, wd=4, c=8, row=0, rows=5, nbytes=1 << 12):
        return lib.srk_lpips_layer_forward(f0, f1, w, n, h, wd, c, row, rows, table, ws, nbytes, None)

    def bwd(f0=p, f1=p, w=p, g=p, df0=p, n=2, h=4, wd=4, c=8):
        return lib.srk_lpips_layer_backward(f0, f1, w, g, n, h, wd, c, df0, None)

    def host(f0=p, f1=p, w=p, g=None, value=p, df0=None, n=2, h=4, wd=4, c=8):
        return lib.srk_lpips_layer_host(f0, f1, w, g, n, h, wd, c, value, df0)

    # (all refused before anything is launched or read: no device is needed for these)
    for call in (fwd, bwd, host):
        assert call(n=0) == -1 and b"bad dims" in err()
        assert call(h=-1) == -1 and call(wd=0) == -1 and call(c=0) == -1
        assert call(f0=None) == -1 and b"null pointer" in err()
        assert call(f1=None) == -1 and call(w=None) == -1
    assert fwd(table=None) == -1 and fwd(ws=None) == -1
    assert fwd(row=5) == -1 and b"row 5 of a table of 5 rows" in err()
    assert fwd(row=-1) == -1 and fwd(rows=0) == -1
    assert fwd(nbytes=8) == -4 and b"workspace" in err()
    assert bwd(g=None) == -1 and bwd(df0=None) == -1
    assert host(value=None) == -1
    assert host(g=p) == -1 and b"given together" in err() and host(df0=p) == -1
    assert lib.srk_lpips_finish(None, 5, 2, 1.0, p, p, None, None) == -1 and b"null pointer" in err()
    assert lib.srk_lpips_finish(p, 5, 2, 1.0, None, None, None, None) == -1
    assert lib.srk_lpips_finish(p, 0, 2, 1.0, p, p, None, None) == -1 and lib.srk_lpips_finish(p, 5, 0, 1.0, p, p, None, None) == -1
    assert lib.srk_lpips_layer_workspace(1, 0, 4, 8) == 0 and lib.srk_lpips_layer_blocks(0, 4, 4, 8, 0) == -1
    assert lib.srk_version() == 600


def test_weight_loading(pkg):
    _, _, lins, vgg_sd, lin_sd = R.filled_net()
    net = pkg.LPIPS()
    assert [i for i, m in enumerate(net.features) if isinstance(m, torch.nn.Conv2d)] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21,
                                                                                         24, 26, 28]
    assert len(net.features) == 30 and [p.numel() for p in net.lins] == list(R.WIDTHS)
    assert all(not p.requires_grad for p in net.parameters())
    assert all(m._cache.frozen for m in net.features if isinstance(m, torch.nn.Conv2d))
    assert net.load_vgg16(vgg_sd) is net and net.load_lins(lin_sd) is net       # extra entries are ignored
    for k, v in vgg_sd.items():
        if k.startswith("features."):
            assert torch.equal(net.state_dict()[k], v), k
    for p, v in zip(net.lins, lins):
        assert torch.equal(p.data, v)
    assert all(not p.requires_grad for p in net.parameters())
    for drop in ("features.28.bias", "features.0.weight"):
        with pytest.raises(KeyError, match=drop.replace(".", r"\.")):
            net.load_vgg16({k: v for k, v in vgg_sd.items() if k != drop})
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        net.load_lins({k: v for k, v in lin_sd.items() if k != "lin3.model.1.weight"})
    with pytest.raises(KeyError):                           # exactly these names: the bare vectors are not accepted
        net.load_lins({"lins.%d" % l: v for l, v in enumerate(lins)})
    with pytest.raises(ValueError, match="lin1"):
        net.load_lins(dict(lin_sd, **{"lin1.model.1.weight": torch.zeros(1, 64, 1, 1)}))
    both = pkg.LPIPS(vgg_sd, lin_sd)
    assert torch.equal(both.features[28].weight, net.features[28].weight) and torch.equal(both.lins[4], net.lins[4])


def test_feature_extractor_layout_is_what_it_was(pkg):
    fe = pkg.FeatureExtractor()
    assert list(fe.state_dict()) == ["features.%d.%s" % (i, s) for i in (0, 2, 5, 7) for s in ("weight", "bias")]
    assert len(fe.features) == 9 and len(pkg.FeatureExtractor(feature_layer=11).features) == 12


def test_mixed_loss_without_the_term_is_the_object_it_was(pkg):
    T, ops = pkg.trainers, pkg.ops
    assert T.mixed_loss(ops.mse_loss, 0, 0, lpips_weight=0) is ops.mse_loss
    assert T.mixed_loss(ops.l1_loss, 0.0, 0.0, "ortho", 0.0, None) is ops.l1_loss
    assert T.mixed_loss(ops.l1_loss, 0.0, 0.0, lpips_weight=0.0, lpips_net=object()) is ops.l1_loss
    assert T.mixed_loss(ops.l1_loss, 0.0, 0.0, lpips_weight=0.1, lpips_net=object()) is not ops.l1_loss
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="lpips_weight"):
            T.mixed_loss(ops.mse_loss, 0, 0, lpips_weight=bad, lpips_net=object())
    with pytest.raises(ValueError, match="lpips_net"):
        T.mixed_loss(ops.mse_loss, 0, 0, lpips_weight=0.1)


def test_trainer_arguments_are_refused_by_name(pkg):
    from pytorch_super_resolution_model_collection_amd.sr_trainers import check_lpips_args
    ok = argparse.Namespace(lpips_vgg="a.pth", lpips_lin="b.pth", lpips_weight=0.1, num_channels=3)
    for kind in ("srcnn", "fsrcnn", "espcn", "vdsr", "edsr", "rcan", "lapsrn"):
        check_lpips_args(ok, kind)
    check_lpips_args(argparse.Namespace(), "edsr")                      # older args objects: nothing asked for
    check_lpips_args(argparse.Namespace(lpips_vgg="a", lpips_lin="b", lpips_weight=0.0, num_channels=3), "srgan")   # metric only
    for kind in ("srgan", "drcn"):
        with pytest.raises(ValueError, match="lpips_weight.*%s" % kind.upper()):
            check_lpips_args(ok, kind)
        with pytest.raises(ValueError, match="lpips_weight"):
            pkg.trainers.build(kind, None, 1e-3, lpips_weight=0.1, lpips_net=object())
    for change, match in ((dict(lpips_lin=None), "lpips_vgg|lpips_lin"), (dict(lpips_vgg=None), "lpips_vgg|lpips_lin"),
                          (dict(lpips_vgg=None, lpips_lin=None), "lpips_weight"), (dict(num_channels=1), "LPIPS reads RGB"),
                          (dict(lpips_weight=-1.0), "lpips_weight")):
        args = argparse.Namespace(**dict(vars(ok), **change))
        with pytest.raises(ValueError, match=match):
            check_lpips_args(args, "edsr")


def test_cli_arguments_are_refused_by_name(tmp_path, capsys):
    import main as cli
    base = ["--model_name", "EDSR", "--save_dir", str(tmp_path)]
    both = ["--lpips_vgg", "a.pth", "--lpips_lin", "b.pth"]
    args = cli.parse_args(base + both + ["--lpips_weight", "0.25"])
    assert (args.lpips_vgg, args.lpips_lin, args.lpips_weight) == ("a.pth", "b.pth", 0.25)
    assert cli.parse_args(base).lpips_weight == 0.0 and cli.parse_args(base).lpips_vgg is None
    cli.parse_args(["--model_name", "SRGAN", "--save_dir", str(tmp_path)] + both)       # the metric alone: any model
    for argv, match in ((base + ["--lpips_vgg", "a.pth"], "come together"), (base + ["--lpips_lin", "b.pth"], "come together"),
                        (base + ["--lpips_weight", "0.1"], "needs --lpips_vgg"),
                        (base + both + ["--num_channels", "1"], "LPIPS reads RGB"),
                        (base + both + ["--lpips_weight", "-0.5"], "number >= 0"),
                        (base + both + ["--lpips_weight", "nan"], "number >= 0"),
                        (["--model_name", "SRGAN", "--save_dir", str(tmp_path)] + both + ["--lpips_weight", "0.1"], "SRGAN has no LPIPS"),
                        (["--model_name", "DRCN", "--save_dir", str(tmp_path)] + both + ["--lpips_weight", "0.1"], "DRCN has no LPIPS")):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
        assert match in capsys.readouterr().err, argv


def test_metric_arguments_are_refused_before_the_device(pkg):
    net = pkg.LPIPS()
    x = torch.zeros(1, 3, 16, 16)
    for pred, target, match in ((torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16), "LPIPS reads RGB"),
                                (torch.zeros(3, 16, 16), torch.zeros(3, 16, 16), "LPIPS reads RGB"),
                                (torch.zeros(1, 3, 15, 16), torch.zeros(1, 3, 15, 16), "at least 16"),
                                (torch.zeros(1, 3, 16, 12), torch.zeros(1, 3, 16, 12), "at least 16"),
                                (x, torch.zeros(1, 3, 16, 17), "pred .* vs target"), (x, x, "on the device")):
        with pytest.raises(ValueError, match=match):
            pkg.ops.lpips(pred, target, net)
    assert pkg.ops.lpips_input_affine(False) == (R.SHIFT, R.SCALE)
    sub, div = pkg.ops.lpips_input_affine(True)
    for c in range(3):      # (x - sub) / div = ((2 x - 1) - shift) / scale
        assert abs((0.3 - sub[c]) / div[c] - ((2 * 0.3 - 1) - R.SHIFT[c]) / R.SCALE[c]) < 1e-12
