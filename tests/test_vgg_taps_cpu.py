"""The multi-layer VGG feature loss without a GPU: the host twins srk_vgg_tap_forward_host / _backward_host (the window
bodies of csrc/vgg_tap_common.h in plain C++, double up to the fp32 stores) against the float64 yardstick of
tests/vgg_taps_ref.py on the whole operator table in all three modes and input kinds, the layer-name table, the refusals
of the layer mapping, the trainer arguments and the command line, the launcher's plan and the exported symbols.  The
device kernels are held to the same table in tests/test_vgg_taps_gpu.py."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import __graft_entry__
import perceptual_ref as P
import vgg_taps_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    return p


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape, mode", R.op_cases(), ids=_id)
def test_host_twins_match_the_yardstick(lib, shape, mode, kind):
    case = R.tap_case(shape, mode, kind)
    loss, ya, yb = R.host_forward(lib, case["a"], case["b"], case["mode"], case["weight"])
    print("srk_vgg_tap_forward_host %s %s %s: loss %.17g ref %.17g" % (shape, mode, kind, loss, case["loss"]))
    assert abs(loss - case["loss"]) <= R.HOST_LOSS_TOL * abs(case["loss"])
    if case["mode"] != R.LAST:
        assert torch.equal(ya, case["ya"]) and torch.equal(yb, case["yb"])        # (no NaN left: every element written)
    da = R.host_backward(lib, case["a"], case["b"], case["g"], case["mode"], case["c"])
    assert not torch.isnan(da).any()
    # the twin forms da in double and stores it as fp32: one rounding of the fp64 value
    err = (da.double() - case["da"]).abs()
    assert bool((err <= R.FP32_EPS * case["da"].abs()).all()), float(err.max())
    # a declared seed or a foreign factor is a factor on c alone
    da3 = R.host_backward(lib, case["a"], case["b"], case["g"], case["mode"], 3.0 * case["c"])
    want3 = R.tap_case(shape, mode, kind, seed_value=3.0)["da"]
    assert bool(((da3.double() - want3).abs() <= R.FP32_EPS * want3.abs()).all())


def test_ties_and_nonpositive_inputs_hold_what_they_are_for():
    a, b = R.tap_inputs((2, 8, 6, 10), "ties")
    assert bool((a == b).any())
    win = torch.nn.functional.unfold(a.reshape(-1, 1, 6, 10), 2, stride=2)      # [planes, 4, windows]
    top = win.max(1, keepdim=True).values
    assert bool((((win == top) & (top > 0)).sum(1) > 1).any())                  # equal positive maxima share a window
    a, _ = R.tap_inputs((2, 8, 6, 10), "nonpositive")
    top = torch.nn.functional.unfold(a.reshape(-1, 1, 6, 10), 2, stride=2).max(1).values
    assert bool((top < 0).any()) and bool((top == 0).any()) and bool((top > 0).any())


def test_equal_maps_give_exact_zeros(lib):
    a, _ = R.tap_inputs((2, 8, 6, 10), "continuous")
    loss, ya, yb = R.host_forward(lib, a, a, R.POOL, 1.0)
    assert loss == 0.0 and torch.equal(ya, yb)
    da = R.host_backward(lib, a, a, torch.zeros(2, 8, 3, 5), R.POOL, 0.25)
    assert float(da.abs().max()) == 0.0


def test_layer_names_follow_the_vgg19_layout(pkg):
    names = pkg.ops.vgg_conv_names(pkg.FeatureExtractor.VGG19_CFG)
    assert pkg.FeatureExtractor.VGG19_CFG == P.VGG19_CFG and names == R.conv_names(P.VGG19_CFG)
    head = P.torch_vgg_head(36)
    assert sorted(names.values()) == [i for i, m in enumerate(head) if isinstance(m, torch.nn.Conv2d)]
    assert all(names[k] == v for k, v in R.REALESRGAN_INDEX.items()) and len(names) == 16
    assert tuple(pkg.ops.REALESRGAN_VGG_LAYERS) == R.REALESRGAN
    plan = pkg.ops.vgg_layer_plan(dict(R.REALESRGAN), P.VGG19_CFG)
    assert plan == [(n, R.REALESRGAN_INDEX[n], w) for n, w in R.REALESRGAN]
    # the order of the head, weight-0 layers dropped
    assert pkg.ops.vgg_layer_plan([("conv5_4", 1), ("conv3_1", 0), ("conv1_2", 2)], P.VGG19_CFG) == \
        [("conv1_2", 2, 2.0), ("conv5_4", 34, 1.0)]


@pytest.mark.parametrize("layers, word", [({"relu1_2": 1.0}, "relu1_2"), ({"conv6_1": 1.0}, "conv6_1"),
                                          ([("conv1_2", 1.0), ("conv1_2", 0.5)], "twice"),
                                          ({"conv2_2": -0.1}, "conv2_2"), ({"conv2_2": float("nan")}, "conv2_2"),
                                          ({"conv2_2": float("inf")}, "conv2_2"), ({"conv2_2": "much"}, "conv2_2"),
                                          ({"conv2_2": 0.0}, "positive"), ({}, "positive")])
def test_layer_mapping_refusals(pkg, layers, word):
    with pytest.raises(ValueError, match=word):
        pkg.ops.vgg_layer_plan(layers, P.VGG19_CFG)


def test_loss_and_module_refusals(pkg):
    fe = pkg.FeatureExtractor(feature_layer=8)
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="'l2'.*not built"):
        pkg.ops.vgg_feature_loss(x, x, fe, {"conv1_2": 1.0}, criterion='l2')
    with pytest.raises(ValueError, match="conv5_4.*feature_layer=34"):
        pkg.ops.vgg_feature_loss(x, x, fe, dict(R.REALESRGAN))
    with pytest.raises(ValueError, match="pred must be"):
        pkg.ops.vgg_feature_loss(torch.zeros(1, 1, 8, 8), x, fe, {"conv1_2": 1.0})
    with pytest.raises(ValueError, match="vs target"):
        pkg.ops.vgg_feature_loss(x, torch.zeros(1, 3, 8, 4), fe, {"conv1_2": 1.0})
    with pytest.raises(ValueError, match="pool1"):
        pkg.utils.VGGFeatureLoss({"pool1": 1.0}, fe)
    m = pkg.utils.VGGFeatureLoss({"conv2_2": 0.5, "conv1_2": 0.0}, fe)
    assert m.layer_weights == {"conv2_2": 0.5} and all(not p.requires_grad for p in m.parameters())
    with pytest.raises(ValueError, match="conv7_7"):
        pkg.trainers.esrgan_segments(None, torch.nn.Linear(1, 1), None, None, fe, vgg_layers={"conv7_7": 1.0})


def test_trainer_argument_checks(pkg):
    from pytorch_super_resolution_model_collection_amd.sr_trainers import check_vgg_layers_args, parse_vgg_layers
    assert parse_vgg_layers(None) is None and check_vgg_layers_args(argparse.Namespace(), "esrgan") is None
    assert [(n, w) for n, _, w in parse_vgg_layers("realesrgan")] == list(R.REALESRGAN)
    assert parse_vgg_layers(" conv3_4:1 , conv1_2:0.25 ") == [("conv1_2", 2, 0.25), ("conv3_4", 16, 1.0)]
    ok = argparse.Namespace(vgg_layers="realesrgan", vgg_weights="v.pth")
    assert [n for n, _, _ in check_vgg_layers_args(ok, "esrgan")] == [n for n, _ in R.REALESRGAN]
    for kind in ("srgan", "edsr", "drcn"):
        with pytest.raises(ValueError, match="vgg_layers.*ESRGAN"):
            check_vgg_layers_args(ok, kind)
    with pytest.raises(ValueError, match="vgg_layers.*vgg_weights"):
        check_vgg_layers_args(argparse.Namespace(vgg_layers="realesrgan", vgg_weights=None), "esrgan")
    for spec, word in (("conv1_2", "name:weight"), ("conv1_2:", "name:weight"), ("conv1_2:x", "conv1_2"),
                       ("conv1_2:1,,conv2_2:1", "name:weight")):
        with pytest.raises(ValueError, match=word):
            parse_vgg_layers(spec)


CLI_REFUSALS = [
    (["--model_name", "ESRGAN", "--vgg_weights", "v.pth", "--vgg_layers", "conv9_9:1"], "conv9_9"),
    (["--model_name", "ESRGAN", "--vgg_weights", "v.pth", "--vgg_layers", "conv1_2:1,conv1_2:2"], "twice"),
    (["--model_name", "ESRGAN", "--vgg_weights", "v.pth", "--vgg_layers", "conv1_2:-1"], "non-negative"),
    (["--model_name", "EDSR", "--vgg_layers", "realesrgan"], "not EDSR"),
    (["--model_name", "SRGAN", "--vgg_weights", "v.pth", "--vgg_layers", "realesrgan"], "not SRGAN"),
    (["--model_name", "ESRGAN", "--vgg_layers", "realesrgan"], "needs --vgg_weights"),
]


def test_command_line(tmp_path):
    """main.py's parser in a child process: every refusal names --vgg_layers and its reason; the accepted forms parse."""
    code = ("import io, json, sys, contextlib\n"
            "sys.path.insert(0, %r)\n"
            "import main as cli\n"
            "base = ['--synthetic', '--save_dir', %r]\n"
            "out = []\n"
            "for argv in json.loads(sys.argv[1]):\n"
            "    err = io.StringIO()\n"
            "    try:\n"
            "        with contextlib.redirect_stderr(err):\n"
            "            args = cli.parse_args(base + argv)\n"
            "        out.append(['ok', args.vgg_layers])\n"
            "    except SystemExit as e:\n"
            "        out.append([e.code, err.getvalue()])\n"
            "print('RESULT ' + json.dumps(out))\n" % (ROOT, str(tmp_path)))
    good = [["--model_name", "ESRGAN", "--vgg_weights", "v.pth", "--vgg_layers", "realesrgan", "--discriminator", "unet",
             "--gan_type", "vanilla", "--ema_decay", "0.9", "--resume"],
            ["--model_name", "ESRGAN", "--vgg_weights", "v.pth", "--vgg_layers", "conv3_4:1,conv5_4:0.5"],
            ["--model_name", "ESRGAN", "--vgg_weights", "v.pth"]]
    r = subprocess.run([sys.executable, "-c", code, json.dumps([a for a, _ in CLI_REFUSALS] + good)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    for (argv, word), (status, text) in zip(CLI_REFUSALS, res):
        assert status == 2 and "--vgg_layers" in text and word in text, (argv, status, text[-300:])
    assert res[len(CLI_REFUSALS):] == [["ok", "realesrgan"], ["ok", "conv3_4:1,conv5_4:0.5"], ["ok", None]]


def test_symbols_plan_and_argument_checks(lib, pkg):
    names = ("srk_vgg_tap_forward", "srk_vgg_tap_backward", "srk_vgg_tap_finish", "srk_vgg_tap_workspace_bytes",
             "srk_vgg_tap_plan", "srk_vgg_tap_forward_host", "srk_vgg_tap_backward_host")
    declared = pkg._lib.header_symbols()
    for name in names:
        assert name in declared and hasattr(lib, name), name
    assert (pkg._lib.VGG_TAP_POOL, pkg._lib.VGG_TAP_RELU, pkg._lib.VGG_TAP_LAST) == (R.POOL, R.RELU, R.LAST)
    assert lib.srk_vgg_tap_workspace_bytes(0) == 0 and lib.srk_vgg_tap_workspace_bytes(5) % 8 == 0
    row = lib.srk_vgg_tap_workspace_bytes(1)
    assert row >= 8 and lib.srk_vgg_tap_workspace_bytes(5) == 5 * row
    # the plan: one block for a small map, a capped grid for a large one, whose blocks then walk several chunks
    for mode in (R.POOL, R.RELU, R.LAST):
        assert R.plan_of(lib, (1, 64, 2, 2), mode, 1)[0] == 1
        assert R.plan_of(lib, (2, 64, 34, 38), mode, 1)[0] > 1
        big, huge = R.plan_of(lib, (4, 64, 512, 512), mode, 1), R.plan_of(lib, (8, 64, 512, 512), mode, 1)
        assert big[0] == huge[0] <= row // 8 and huge[2] > big[2] > 1
    n, c, h, w = R.multi_chunk_shape(lib)
    assert R.plan_of(lib, (n, c, h, w), R.POOL, 1)[2] == 2 and R.plan_of(lib, (n, c, h - 2, w - 2), R.POOL, 1)[2] == 1
    assert R.plan_of(lib, (n, c, h, w), R.POOL, 0)[2] >= 2        # the 4-byte path at the same shape as well
    assert lib.srk_vgg_tap_plan(1, 4, 4, 6, R.POOL, 1, None) == -1 and b"C % 4" in lib.srk_last_error_string()
    assert lib.srk_vgg_tap_plan(1, 1, 4, 8, R.POOL, 1, None) == -1 and b"2 x 2 window" in lib.srk_last_error_string()
    assert lib.srk_vgg_tap_plan(1, 1, 1, 8, R.LAST, 1, None) == 1
    # refusals come before anything is read or launched: no device is needed for these
    buf = torch.zeros(1 << 12, dtype=torch.float64)
    p = ctypes.c_void_p(buf.data_ptr())
    err = lambda: lib.srk_last_error_string()

    def fwd(a=p, b=p, ws=p, ya=p, yb=p, n=1, h=4, w=4, c=8, mode=R.POOL, weight=1.0, row=0, rows=1):
        return lib.srk_vgg_tap_forward(a, b, n, h, w, c, mode, weight, row, rows, ws, ya, yb, None)

    def bwd(a=p, b=p, g=p, da=p, n=1, h=4, w=4, c=8, mode=R.POOL, cv=1.0):
        return lib.srk_vgg_tap_backward(a, b, g, n, h, w, c, mode, cv, None, da, None)

    def hfwd(a=p, b=p, loss=ctypes.pointer(ctypes.c_double(0.0)), ya=p, yb=p, n=1, h=4, w=4, c=8, mode=R.POOL, weight=1.0):
        return lib.srk_vgg_tap_forward_host(a, b, n, h, w, c, mode, weight, loss, ya, yb)

    def hbwd(a=p, b=p, g=p, da=p, n=1, h=4, w=4, c=8, mode=R.POOL):
        return lib.srk_vgg_tap_backward_host(a, b, g, n, h, w, c, mode, 1.0, da)

    for call in (fwd, bwd, hfwd, hbwd):
        assert call(n=0) == -1 and b"bad dims" in err()
        assert call(h=-1) == -1 and call(w=0) == -1 and call(c=0) == -1
        assert call(a=None) == -1 and b"null pointer" in err()
        assert call(b=None) == -1
        assert call(mode=3) == -1 and b"mode 3" in err()
        assert call(h=1) == -1 and b"2 x 2 window" in err()
    assert fwd(ws=None) == -1 and fwd(ya=None) == -1 and fwd(yb=None) == -1 and hfwd(ya=None) == -1
    assert fwd(weight=-1.0) == -1 and b"weight" in err() and hfwd(weight=float("nan")) == -1
    assert fwd(row=1) == -1 and b"row 1 of a workspace of 1 rows" in err() and fwd(row=-1) == -1 and fwd(rows=0) == -1
    assert bwd(g=None) == -1 and bwd(da=None) == -1 and hbwd(g=None) == -1 and hbwd(da=None) == -1
    assert bwd(cv=float("inf")) == -1 and b"finite" in err()
    assert lib.srk_vgg_tap_finish(None, 1, p, None) == -1 and lib.srk_vgg_tap_finish(p, 1, None, None) == -1
    assert lib.srk_vgg_tap_finish(p, 0, p, None) == -1
    assert lib.srk_version() == 600
