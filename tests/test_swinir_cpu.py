"""SwinIR without a GPU: srk_window_attention_host (the loop and the index arithmetic of csrc/wattn_common.h, in plain C++
double) against the fp64 restatement of tests/swinir_ref.py over its case table, the header's region-id and
relative-index functions against the restatement's tensors exactly, the net's keys and shapes, the command line and
every refusal.  The device kernels are held to the same table in tests/test_wattn_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__
import swinir_ref as R

# both sides are fp64 on the same fp32 inputs: only summation order and exp() differ
HOST_TOL = 1e-12


@pytest.fixture(scope="module")
def lib():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    return p._lib.load()


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


@pytest.mark.parametrize("name", list(R.CASES))
def test_host_twin_matches_restatement(lib, name):
    case = R.CASES[name]
    want, got = R.attention_with_grads(case), R.host(lib, case)
    for what, a, b in zip(("out", "dqkv", "dtable"), (got.out, got.dqkv, got.dtable), want):
        err = R.worst(a, b)
        print("srk_window_attention_host %-16s %-6s worst %.3g of max |ref|" % (name, what, err))
        assert err <= HOST_TOL, (name, what, err)


def test_host_forward_only(lib):
    case = R.CASES["9_tokens"]
    assert torch.equal(R.host(lib, case, backward=False).out, R.host(lib, case).out)


@pytest.mark.parametrize("name", list(R.CASES))
def test_region_ids_and_pixels_are_the_restatements(lib, name):
    """Exactly: the mask built from the header's region ids is the restatement's mask tensor, and the pixel a window's
    token is read from is where roll + partition put it."""
    n, h, w, c, heads, window, shift = R.CASES[name]
    t = window * window
    if shift:
        img = R.region_image(h, w, window, shift)
        mine = torch.tensor([[lib.srk_window_attention_region(h, w, window, shift, r, cc) for cc in range(w)]
                             for r in range(h)])
        assert torch.equal(mine, img)
        ids = R.partition(mine[None, :, :, None], window)[:, :, 0]
        mask = torch.where(ids[:, :, None] != ids[:, None, :], -100.0, 0.0).double()
        assert torch.equal(mask, R.mask_tensor(h, w, window, shift))
    else:
        assert lib.srk_window_attention_region(h, w, window, 0, h - 1, w - 1) == 0
    pix = torch.arange(h * w).view(1, h, w, 1)
    wins = R.partition(torch.roll(pix, (-shift, -shift), (1, 2)), window)[:, :, 0]          # windows, T
    for wy in range(h // window):
        for wx in range(w // window):
            mine = [lib.srk_window_attention_token_pixel(h, w, window, shift, wy, wx, k) for k in range(t)]
            assert mine == wins[wy * (w // window) + wx].tolist()


@pytest.mark.parametrize("window", range(2, 9))
def test_relative_index_is_the_restatements(lib, window):
    t = window * window
    mine = torch.tensor([[lib.srk_window_attention_rel_index(window, i, j) for j in range(t)] for i in range(t)])
    assert torch.equal(mine, R.rel_index(window))
    assert int(mine.min()) == 0 and int(mine.max()) == (2 * window - 1) ** 2 - 1


def test_argument_checks(lib):
    buf = np.zeros(1 << 16, np.float32)
    out = np.zeros(1 << 16, np.float64)
    p, o = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    err = lambda: lib.srk_last_error_string()

    def host(qkv=p, y=o, n=1, h=4, w=4, c=4, heads=1, window=4, shift=0, g=None):
        return lib.srk_window_attention_host(qkv, p, g, n, h, w, c, heads, window, shift, y, None, None)

    def fwd(n=1, h=4, w=4, c=4, heads=1, window=4, shift=0, qkv=p):
        return lib.srk_window_attention_forward(qkv, p, n, h, w, c, heads, window, shift, p, None, None)

    def bwd(n=1, h=4, w=4, c=4, heads=1, window=4, shift=0, qkv=p):
        return lib.srk_window_attention_backward(p, qkv, p, p, p, n, h, w, c, heads, window, shift, p, None, 0.0, None, 0,
                                                 None)

    # (all refused before anything is launched or read: no device is needed for these)
    for call in (host, fwd, bwd):
        assert call(n=0) == -1 and b"bad dims" in err()
        assert call(window=9, h=9, w=9) == -1 and b"window 9" in err()
        assert call(window=1) == -1 and b"window 1" in err()
        assert call(shift=4) == -1 and b"shift 4" in err()
        assert call(shift=-1) == -1
        assert call(h=6) == -1 and b"6 x 4 is not a multiple of the window 4" in err()
        assert call(c=6, heads=4) == -1 and b"4 heads do not divide C = 6" in err()
        assert call(c=33) == -1 and b"head dimension 33, at most 32" in err()
        assert call(qkv=None) == -1 and b"null pointer" in err()
    assert host(g=p) == -1 and b"a backward needs" in err()
    assert lib.srk_window_attention_backward(p, p, p, p, p, 1, 4, 4, 4, 1, 4, 0, p, p, 0.0, None, 0, None) == -1
    assert lib.srk_window_attention_backward(p, p, p, p, p, 1, 4, 4, 4, 1, 4, 0, p, p, 0.0, p, 8, None) == -4
    assert b"workspace" in err()
    assert lib.srk_window_attention_workspace(2, 8, 12, 8, 2, 4) == 12 * 2 * 49 * 4
    assert lib.srk_window_attention_workspace(1, 6, 8, 8, 2, 4) == 0
    assert lib.srk_layer_norm_workspace(0, 8) == 0 and lib.srk_layer_norm_workspace(100, 8) == 7 * 2 * 8 * 4
    assert lib.srk_layer_norm_forward(p, p, p, p, None, None, 0, 8, 1e-5, None) == -1 and b"bad dims" in err()
    assert lib.srk_layer_norm_forward(p, p, p, p, p, None, 4, 8, 1e-5, None) == -1 and b"saved together" in err()
    assert lib.srk_layer_norm_backward(p, p, p, p, p, None, None, None, 0.0, 4, 8, None, 0, None) == -1
    assert lib.srk_gelu_forward(p, None, 4, None) == -1 and lib.srk_gelu_backward(p, p, p, 0, None) == -1
    assert lib.srk_version() == 600


def test_header_symbols_find_the_new_entry_points():
    names = _pkg()._lib.header_symbols()
    for s in ("srk_window_attention_forward", "srk_window_attention_backward", "srk_window_attention_host",
              "srk_window_attention_workspace", "srk_layer_norm_forward", "srk_layer_norm_backward", "srk_gelu_forward",
              "srk_gelu_backward"):
        assert s in names, s


CLASSICAL = (3, 180, (6, 6, 6, 6, 6, 6), 6, 8, 2, 4, "pixelshuffle")
LIGHTWEIGHT = (3, 60, (6, 6, 6, 6), 6, 8, 2, 2, "pixelshuffledirect")


@pytest.mark.parametrize("ctor", [CLASSICAL, LIGHTWEIGHT, (1, 16, (2, 1), 2, 4, 2, 3, "pixelshuffle"),
                                  (3, 16, (1,), 2, 4, 1.5, 8, "pixelshuffle")], ids=["classical", "lightweight", "x3", "x8"])
def test_state_dict_is_the_plain_nets(ctor):
    """Keys and shapes are those of the plain-torch SwinIR of tests/swinir_ref.py, which loads the package's state_dict."""
    net = _pkg().SwinIRNet(*ctor)
    ref = R.ref_swinir_like(net, *ctor)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == want
    assert not any("relative_position_index" in k or "attn_mask" in k for k in want)
    dim, heads, window = ctor[1], ctor[3], ctor[4]
    hidden = int(dim * ctor[5])
    pre = "layers.%d.residual_group.blocks.%d." % (len(ctor[2]) - 1, ctor[2][-1] - 1)
    assert want[pre + "attn.relative_position_bias_table"] == ((2 * window - 1) ** 2, heads)
    assert want[pre + "attn.qkv.weight"] == (3 * dim, dim) and want[pre + "attn.proj.weight"] == (dim, dim)
    assert want[pre + "mlp.fc1.weight"] == (hidden, dim) and want[pre + "mlp.fc2.weight"] == (dim, hidden)
    assert want[pre + "norm1.weight"] == want[pre + "norm2.bias"] == want["norm.weight"] == want["patch_embed.norm.bias"] == (dim,)
    assert want["conv_first.weight"] == (dim, ctor[0], 3, 3) and want["conv_after_body.weight"] == (dim, dim, 3, 3)
    assert want["layers.0.conv.weight"] == (dim, dim, 3, 3)
    if ctor[7] == "pixelshuffle":
        assert want["conv_before_upsample.0.weight"] == (64, dim, 3, 3) and want["conv_last.weight"] == (ctor[0], 64, 3, 3)
        assert want["upsample.0.weight"] == ((9 if ctor[6] == 3 else 4) * 64, 64, 3, 3)
        assert ("upsample.2.weight" in want) == (ctor[6] in (4, 8)) and ("upsample.4.weight" in want) == (ctor[6] == 8)
    else:
        assert want["upsample.0.weight"] == (ctor[6] ** 2 * ctor[0], dim, 3, 3) and "conv_last.weight" not in want


def test_parameter_counts_and_shifts():
    pkg = _pkg()
    net = pkg.SwinIRNet(*CLASSICAL)
    assert sum(p.numel() for p in net.parameters()) == 11900199
    shifts = [b.shift_size for b in net.layers[2].residual_group.blocks]
    assert shifts == [0, 4, 0, 4, 0, 4]
    assert pkg.SwinIRNet(*LIGHTWEIGHT).mean == (0.4488, 0.4371, 0.4040) and pkg.SwinIRNet(1, 16, (1,), 2, 4).mean is None


def test_net_refuses_bad_arguments():
    pkg = _pkg()
    with pytest.raises(ValueError, match="upsampler 'nearest\\+conv'"):
        pkg.SwinIRNet(3, 16, (1,), 2, 4, 2, 4, "nearest+conv")
    with pytest.raises(ValueError, match="scale_factor 5"):
        pkg.SwinIRNet(3, 16, (1,), 2, 4, 2, 5, "pixelshuffle")
    with pytest.raises(ValueError, match="depths"):
        pkg.SwinIRNet(3, 16, (), 2, 4)
    with pytest.raises(ValueError, match="3 heads do not divide 16"):
        pkg.SwinIRNet(3, 16, (1,), 3, 4)
    with pytest.raises(ValueError, match="head dimension 64"):
        pkg.SwinIRNet(3, 64, (1,), 1, 4)
    with pytest.raises(ValueError, match="window 16"):
        pkg.SwinIRNet(3, 16, (1,), 2, 16)
    net = pkg.SwinIRNet(3, 16, (1,), 2, 4, 2, 2).train()
    with pytest.raises(ValueError, match="10 x 13 input is not a multiple of the window 4"):
        net(torch.zeros(1, 3, 10, 13))
    with pytest.raises(RuntimeError, match="GPU"):      # no CPU fallback once the shape is accepted
        net(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="shift 4"):
        pkg.ops.window_attention(torch.zeros(1, 4, 4, 12), torch.zeros(49, 2), 2, 4, 4)


def test_eval_padding_is_reflect_at_bottom_and_right():
    net = _pkg().SwinIRNet(3, 16, (1,), 2, 4, 2, 2).eval()
    x = torch.rand(2, 3, 10, 13)
    assert torch.equal(net.check_image_size(x), torch.nn.functional.pad(x, (0, 3, 0, 2), mode="reflect"))
    assert net.check_image_size(x[:, :, :8, :12]) is not None and net.check_image_size(x[:, :, :8, :12]).shape[2:] == (8, 12)


def test_tiling_refuses_window_attention():
    from pytorch_super_resolution_model_collection_amd import tiling
    net = _pkg().SwinIRNet(3, 16, (2, 2), 2, 4, 2, 2).eval()
    with pytest.raises(ValueError) as e:
        tiling.net_geometry(net)
    assert str(e.value) == ("layers.0.residual_group.blocks.0.attn: WindowAttention partitions the whole image into "
                            "windows and cannot be tiled")


def test_cli(tmp_path, capsys):
    import main
    base = ["--save_dir", str(tmp_path / "r"), "--model_name", "SwinIR", "--scale_factor", "4", "--crop_size", "192"]
    a = main.parse_args(base)
    assert (a.swinir_dim, a.swinir_depths, a.swinir_heads, a.swinir_window, a.swinir_mlp_ratio, a.swinir_upsampler) == \
        (180, (6, 6, 6, 6, 6, 6), 6, 8, 2.0, "pixelshuffle")
    a = main.parse_args(base + ["--swinir_dim", "60", "--swinir_depths", "6,6,6,6", "--swinir_upsampler",
                                "pixelshuffledirect", "--ssim_weight", "0.2", "--ema_decay", "0.9", "--self_ensemble",
                                "--eager", "--degrade", "--fft_weight", "0.1"])
    assert (a.swinir_dim, a.swinir_depths, a.swinir_upsampler, a.ssim_weight) == (60, (6, 6, 6, 6), "pixelshuffledirect", 0.2)
    for flag, bads in (("--swinir_dim", ("0", "x")), ("--swinir_depths", ("0", "6,,6", "a")), ("--swinir_heads", ("0",)),
                       ("--swinir_window", ("0", "1", "9")), ("--swinir_mlp_ratio", ("0", "-1", "nan", "x")),
                       ("--swinir_upsampler", ("nearest+conv",))):
        for bad in bads:
            with pytest.raises(SystemExit):
                main.parse_args(base + [flag, bad])
            assert flag in capsys.readouterr().err, (flag, bad)
    for extra, word in ((["--swinir_heads", "7"], "--swinir_heads 7 does not divide --swinir_dim 180"),
                        (["--swinir_heads", "4"], "head dimension of 45 exceeds 32"),
                        (["--crop_size", "200"], "--crop_size 200 / --scale_factor 4 is not a multiple of --swinir_window 8"),
                        (["--crop_size", "194"], "--crop_size 194"),
                        (["--scale_factor", "5", "--crop_size", "200"], "--scale_factor 5"),
                        (["--tile", "64"], "WindowAttention"), (["--tile", "auto"], "--tile")):
        with pytest.raises(SystemExit):
            main.parse_args(["--save_dir", str(tmp_path / "t")] + base[2:] + extra)
        assert word in capsys.readouterr().err, extra
    assert not (tmp_path / "t").exists()          # refused at argument checking: nothing was set up
    # other models neither gain nor lose anything
    assert main.parse_args(["--save_dir", str(tmp_path / "e"), "--model_name", "EDSR", "--tile", "64"]).tile == 64


def test_trainer_table_and_tile_refusal():
    """The trainer class refuses an args object that carries a tile before it touches a device."""
    from types import SimpleNamespace
    from pytorch_super_resolution_model_collection_amd import sr_trainers, optim, trainers
    assert sr_trainers.TRAINERS["SwinIR"].kind == "swinir"
    with pytest.raises(ValueError, match="WindowAttention"):
        sr_trainers.TRAINERS["SwinIR"](SimpleNamespace(model_name="SwinIR", tile=64))
    assert "swinir" in trainers.build.__doc__
