"""Real-ESRGAN's discriminator without a GPU: the three host twins (srk_spectral_norm_host, srk_upsample_bilinear2x_host,
srk_gan_logit_loss_host: the kernels' own headers in double) against fp64 torch over the case tables of
tests/realesrgan_ref.py, the state_dict of UNetDiscriminatorSN against torch's own spectral_norm, the exported symbols and
the refusals of the command line, the trainer and the C entry points."""
import argparse
import ctypes

import pytest
import torch

import realesrgan_ref as RR

# fp64 on both sides: the two differ by summation order only (tests/test_ragan_cpu.py's tolerance)
TOL = 1e-9


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _pkg()._lib.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _close(got, want, tol=TOL):
    return RR.worst(got.reshape(want.shape), want) <= tol


def _close_dw(got, want, g, sigma, tol=TOL):
    """dW = (G - <G, w_sn> u v^T) / sigma is a difference of two terms of size |G| / sigma, and for R = 1 or K = 1 it is
    zero but for their rounding: the error is held to that size where the result itself is smaller."""
    scale = max(float(want.abs().max()), float(g.abs().max()) / abs(sigma))
    return float((got.reshape(want.shape) - want).abs().max()) <= tol * scale


# ---- spectral normalisation ---------------------------------------------------------------------------------------------
def _sn_host(lib, w, u, v, training, g=None):
    """One host call; u and v (double) are updated in place.  -> (rc, w_sn, sigma, dW)."""
    r, k = w.shape[0], w.numel() // w.shape[0]
    w_sn = torch.full((r, k), float("nan"), dtype=torch.float64)
    dw = torch.full((r, k), float("nan"), dtype=torch.float64) if g is not None else None
    sigma = ctypes.c_double(float("nan"))
    g64 = g.double().contiguous() if g is not None else None
    rc = lib.srk_spectral_norm_host(_p(w), r, k, int(training), RR.EPS, _p(u), _p(v), _p(w_sn), ctypes.byref(sigma),
                                    _p(g64), _p(dw))
    return rc, w_sn, sigma.value, dw


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", RR.SN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spectral_norm_host_matches_torch(lib, shape, training):
    w, u, v = RR.sn_case(shape, 400 + shape[0])
    g = RR.randn(shape, 77)
    want = RR.sn_reference(w, u, v, training, g)
    u64, v64 = u.double().clone(), v.double().clone()
    rc, w_sn, sigma, dw = _sn_host(lib, w, u64, v64, training, g)
    assert rc == 0
    assert torch.isfinite(w_sn).all() and torch.isfinite(dw).all() and sigma == sigma
    assert _close(u64, want["u"]) and _close(v64, want["v"])
    assert abs(sigma - want["sigma"]) <= TOL * abs(want["sigma"])
    assert _close(w_sn, want["w_sn"]) and _close_dw(dw, want["dW"], g, sigma)
    if not training:        # eval mode leaves the buffers alone
        assert torch.equal(u64, u.double()) and torch.equal(v64, v.double())


def test_two_forwards_then_both_backwards(lib):
    """Two training-mode forwards between two optimizer steps, then both backwards: each uses the u, v, sigma of ITS
    forward.  torch keeps them in the graph (clones); the host twin's backward is its eval-mode call on the kept copies."""
    shape = (16, 3, 4, 4)
    w, u, v = RR.sn_case(shape, 91)
    g1, g2 = RR.randn(shape, 5), RR.randn(shape, 6)
    m = RR.sn_module(w, u, v)
    m.train()
    w1 = m.weight()
    w2 = m.weight()
    d1, = torch.autograd.grad((w1 * g1.double()).sum(), m.conv.weight_orig)
    d2, = torch.autograd.grad((w2 * g2.double()).sum(), m.conv.weight_orig)
    u64, v64 = u.double().clone(), v.double().clone()
    rc, h1, s1, _ = _sn_host(lib, w, u64, v64, True)
    u1, v1 = u64.clone(), v64.clone()
    rc2, h2, s2, _ = _sn_host(lib, w, u64, v64, True)
    u2, v2 = u64.clone(), v64.clone()
    assert rc == 0 and rc2 == 0 and s1 != s2 and not torch.equal(u1, u2)
    assert _close(h1, w1.detach()) and _close(h2, w2.detach())
    assert _close(u2, m.conv.weight_u) and _close(v2, m.conv.weight_v)
    _, _, _, b1 = _sn_host(lib, w, u1, v1, False, g1)
    _, _, _, b2 = _sn_host(lib, w, u2, v2, False, g2)
    assert _close_dw(b1, d1, g1, s1) and _close_dw(b2, d2, g2, s2)
    # with the other forward's copies the gradient is another one: the node must keep its own
    _, _, _, wrong = _sn_host(lib, w, u2, v2, False, g1)
    assert not _close(wrong, d1, 1e-6)


def test_spectral_norm_refusals(lib):
    w = torch.zeros(4, 6)
    u, v, out = torch.zeros(4, dtype=torch.float64), torch.zeros(6, dtype=torch.float64), torch.zeros(24, dtype=torch.float64)
    s = ctypes.c_double()
    host = lib.srk_spectral_norm_host
    assert host(None, 4, 6, 1, 1e-12, _p(u), _p(v), _p(out), ctypes.byref(s), None, None) == -1
    assert host(_p(w), 0, 6, 1, 1e-12, _p(u), _p(v), _p(out), ctypes.byref(s), None, None) == -1
    assert "R = 0" in lib.srk_last_error_string().decode()
    assert host(_p(w), 4, -1, 1, 1e-12, _p(u), _p(v), _p(out), ctypes.byref(s), None, None) == -1
    assert host(_p(w), 4, 6, 1, 1e-12, _p(u), _p(v), _p(out), ctypes.byref(s), _p(out), None) == -1
    assert "come together" in lib.srk_last_error_string().decode()
    # the device entry points refuse before they launch anything
    L = _pkg()._lib
    one = L.SpectralLayer(w.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr(), None, 4, 6)
    table = (L.SpectralLayer * 1)(one)
    assert lib.srk_spectral_norm_forward(table, 0, 1, 1e-12, _p(w), 1 << 20, None) == -1
    assert lib.srk_spectral_norm_forward(table, 17, 1, 1e-12, _p(w), 1 << 20, None) == -1
    assert "17 layers" in lib.srk_last_error_string().decode()
    assert lib.srk_spectral_norm_forward(table, 1, 1, 1e-12, None, 0, None) == -1
    assert lib.srk_spectral_norm_forward(table, 1, 1, 1e-12, _p(w), 8, None) == -1
    assert "workspace" in lib.srk_last_error_string().decode()
    big = (L.SpectralLayer * 1)(L.SpectralLayer(w.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr(), None, 4, 16385))
    assert lib.srk_spectral_norm_forward(big, 1, 1, 1e-12, _p(w), 1 << 30, None) == -1
    assert "16385" in lib.srk_last_error_string().decode()
    assert lib.srk_spectral_norm_workspace(table, 1) == (6 + 4) * 8      # t = W^T u and s = W v, in double
    assert lib.srk_spectral_norm_backward(None, _p(w), _p(w), 4, 6, _p(w), 0.0, _p(w), 64, None) == -1
    assert lib.srk_spectral_norm_backward(_p(w), _p(w), _p(w), 4, 6, _p(w), 0.0, _p(w), 0, None) == -1
    assert lib.srk_spectral_norm_backward_workspace(4, 6) == 8 and lib.srk_spectral_norm_backward_workspace(64, 65) == 16


# ---- bilinear x2 ------------------------------------------------------------------------------------------------------------
def _bl_host(lib, x, add, dy):
    n, h, w, c = x.shape
    y = torch.full((n, 2 * h, 2 * w, c), float("nan"), dtype=torch.float64)
    dx = torch.full((n, h, w, c), float("nan"), dtype=torch.float64) if dy is not None else None
    rc = lib.srk_upsample_bilinear2x_host(_p(x), _p(add), _p(dy), n, h, w, c, _p(y), _p(dx))
    return rc, y, dx


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("shape", RR.BILINEAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bilinear_host_matches_interpolate(lib, shape, with_add):
    n, h, w, c = shape
    x = RR.randn(shape, 11)
    add = RR.randn(shape, 12) if with_add else None
    dy = RR.randn((n, 2 * h, 2 * w, c), 13)
    want_y, want_dx = RR.bilinear_reference(x, add, dy)
    rc, y, dx = _bl_host(lib, x, add, dy)
    assert rc == 0 and torch.isfinite(y).all() and torch.isfinite(dx).all()
    assert _close(y, want_y) and _close(dx, want_dx)
    # the adjoint identity <up(x), g> = <x, up^T(g)> (x alone: the map is linear)
    _, y0, _ = _bl_host(lib, x, None, None)
    lhs, rhs = float((y0 * dy.double()).sum()), float((x.double() * dx).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(float((y0 * dy.double()).abs().sum()), 1e-300)


def test_bilinear_index_rule(lib):
    """A row of n = 3 values 0, 4, 8: output 2k reads (k - 1, k) with (0.25, 0.75), index 0 alone for k = 0; output 2k + 1
    reads (k, min(k + 1, n - 1)) with (0.75, 0.25)."""
    x = torch.tensor([0.0, 4.0, 8.0]).reshape(1, 1, 3, 1)
    _, y, _ = _bl_host(lib, x, None, None)
    assert y[0, 0, :, 0].tolist() == [0.0, 1.0, 3.0, 5.0, 7.0, 8.0] and torch.equal(y[0, 0], y[0, 1])


def test_bilinear_refusals(lib):
    x = torch.zeros(8)
    y = torch.zeros(64, dtype=torch.float64)
    host = lib.srk_upsample_bilinear2x_host
    assert host(_p(x), None, None, 1, 0, 2, 1, _p(y), None) == -1
    assert "H = 0" in lib.srk_last_error_string().decode()
    assert host(_p(x), None, None, 1, 2, 2, 1, None, None) == -1
    assert host(None, None, None, 1, 2, 2, 1, None, None) == -1
    assert host(None, _p(x), _p(x), 1, 2, 2, 1, None, _p(y)) == -1
    assert lib.srk_upsample_bilinear2x_forward(None, None, _p(x), 1, 1, 1, 1, None) == -1
    assert lib.srk_upsample_bilinear2x_forward(_p(x), None, _p(x), 1, 1, -1, 1, None) == -1
    assert lib.srk_upsample_bilinear2x_backward(_p(x), None, 1, 1, 1, 1, None) == -1
    assert lib.srk_upsample_bilinear2x_backward(_p(x), _p(x), 0, 1, 1, 1, None) == -1


# ---- the vanilla GAN loss on logits --------------------------------------------------------------------------------------------
def _gan_host(lib, x, real, scale=1.0, want_grad=True):
    loss = ctypes.c_double(float("nan"))
    dx = torch.full((x.numel(),), float("nan"), dtype=torch.float64) if want_grad else None
    rc = lib.srk_gan_logit_loss_host(_p(x), x.numel(), int(real), scale, ctypes.byref(loss), _p(dx))
    return rc, loss.value, dx


@pytest.mark.parametrize("real", [True, False])
@pytest.mark.parametrize("extreme", [False, True])
@pytest.mark.parametrize("n", RR.GAN_SIZES)
def test_gan_logit_host_matches_autograd(lib, n, extreme, real):
    x = RR.gan_logits(n, 300 + n, extreme)
    want, wdx = RR.gan_reference(x, real)
    rc, loss, dx = _gan_host(lib, x, real)
    assert rc == 0 and loss == loss and torch.isfinite(dx).all()
    assert abs(loss - float(want)) <= TOL * abs(float(want)) and _close(dx, wdx)
    # BasicSR's form of the same number (torch's kernel takes log(1 + exp(-|x|)) without log1p: an absolute error of one
    # rounding of 1 per element, which is all that is left of a saturated logit's term)
    assert abs(loss - float(RR.gan_loss(x.double(), real))) <= TOL * abs(float(want)) + 1e-15
    # the seed scales the gradient and leaves the loss alone; no gradient row is a NULL pointer
    rc, loss2, dx2 = _gan_host(lib, x, real, scale=0.005)
    assert rc == 0 and loss2 == loss and _close(dx2, 0.005 * wdx)
    rc, loss3, none = _gan_host(lib, x, real, want_grad=False)
    assert rc == 0 and loss3 == loss and none is None


def test_gan_logit_saturates(lib):
    x = torch.tensor([60.0, -60.0])
    _, lr, dr = _gan_host(lib, x, True)
    _, lf, df = _gan_host(lib, x, False)
    assert abs(lr - 30.0) <= 1e-12 * 30 and abs(lf - 30.0) <= 1e-12 * 30
    assert abs(float(dr[1]) + 0.5) <= 1e-12 and abs(float(df[0]) - 0.5) <= 1e-12


def test_gan_logit_refusals(lib):
    x = torch.zeros(4)
    loss = ctypes.c_double()
    assert lib.srk_gan_logit_loss_host(_p(x), 0, 1, 1.0, ctypes.byref(loss), None) == -1
    assert "n = 0" in lib.srk_last_error_string().decode()
    assert lib.srk_gan_logit_loss_host(None, 4, 1, 1.0, ctypes.byref(loss), None) == -1
    assert lib.srk_gan_logit_loss_host(_p(x), 4, 1, 1.0, None, None) == -1
    assert lib.srk_gan_logit_loss_forward_backward(_p(x), 0, 1, 1.0, _p(x), None, _p(x), None) == -1
    assert lib.srk_gan_logit_loss_forward_backward(_p(x), 4, 1, 1.0, _p(x), None, None, None) == -1
    assert lib.srk_gan_logit_loss_workspace_bytes() >= 8


# ---- the net's surface -----------------------------------------------------------------------------------------------------------
def test_state_dict_is_torchs():
    pkg = _pkg()
    net = pkg.UNetDiscriminatorSN(3, 8)
    ref = RR.RefUNetDiscriminatorSN(3, 8)
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert got == want == RR.state_table(3, 8)
    assert list(net.state_dict()) == list(ref.state_dict())
    for k in ("conv1.weight_orig", "conv1.weight_u", "conv1.weight_v"):
        assert k in got
    assert [n for n, _ in net.named_parameters()] == [n for n, _ in ref.named_parameters()]
    # each loads the other's file; u and v start as unit vectors
    net.load_state_dict(ref.state_dict())
    ref.load_state_dict(net.state_dict())
    fresh = pkg.UNetDiscriminatorSN(3, 8)
    for name, b in fresh.named_buffers():
        assert abs(float(b.double().norm()) - 1.0) <= 1e-6, name
    assert pkg.UNetDiscriminatorSN(1, 4, skip_connection=False).skip_connection is False


def test_size_refusal_names_the_number():
    net = _pkg().UNetDiscriminatorSN(3, 8)
    with pytest.raises(ValueError, match="12"):
        net(torch.zeros(2, 3, 12, 16))
    with pytest.raises(ValueError, match="W = 20"):
        net(torch.zeros(2, 3, 16, 20))
    with pytest.raises(ValueError, match="shape"):
        net(torch.zeros(2, 1, 16, 16))


def test_symbols_are_declared_and_exported(lib):
    L = _pkg()._lib
    declared = L.header_symbols()
    for n in ("srk_spectral_norm_workspace", "srk_spectral_norm_forward", "srk_spectral_norm_backward_workspace",
              "srk_spectral_norm_backward", "srk_spectral_norm_host", "srk_upsample_bilinear2x_forward",
              "srk_upsample_bilinear2x_backward", "srk_upsample_bilinear2x_host", "srk_gan_logit_loss_workspace_bytes",
              "srk_gan_logit_loss_forward_backward", "srk_gan_logit_loss_host"):
        assert n in declared and n in L._PROTOTYPES and hasattr(lib, n), n
    assert lib.srk_version() == 600
    ops = _pkg().ops
    assert callable(ops.spectral_norm) and callable(ops.upsample_bilinear2x) and callable(ops.gan_logit_loss)
    assert ctypes.sizeof(L.SpectralLayer) == 48


# ---- the command line and the trainer ----------------------------------------------------------------------------------------
BASE = ["--model_name", "ESRGAN", "--synthetic", "--vgg_weights", "vgg.pth", "--crop_size", "32"]


def _parse(tmp_path, *flags, base=BASE):
    import main as cli
    return cli.parse_args(list(base) + ["--save_dir", str(tmp_path)] + list(flags))


def test_cli_defaults(tmp_path):
    a = _parse(tmp_path)
    assert (a.discriminator, a.gan_type, a.unet_feat) == ("vgg", "ragan", None)
    a = _parse(tmp_path, "--discriminator", "unet")
    assert (a.discriminator, a.gan_type, a.unet_feat) == ("unet", "vanilla", 64)
    a = _parse(tmp_path, "--discriminator", "unet", "--unet_feat", "16", "--gan_type", "vanilla")
    assert a.unet_feat == 16
    assert _parse(tmp_path, "--gan_type", "vanilla").discriminator == "vgg"
    other = _parse(tmp_path, base=["--model_name", "EDSR", "--synthetic"])
    assert (other.discriminator, other.gan_type, other.unet_feat) == (None, None, None)


@pytest.mark.parametrize("flags, word", [
    (("--discriminator", "unet", "--gan_type", "ragan"), "--gan_type"),
    (("--discriminator", "unet", "--crop_size", "36"), "--crop_size"),
    (("--unet_feat", "16"), "--unet_feat"),
    (("--discriminator", "resnet"), "--discriminator"),
    (("--gan_type", "lsgan"), "--gan_type"),
    (("--discriminator", "unet", "--unet_feat", "0"), "--unet_feat"),
])
def test_cli_refusals(tmp_path, capsys, flags, word):
    with pytest.raises(SystemExit):
        _parse(tmp_path, *flags)
    assert word in capsys.readouterr().err


@pytest.mark.parametrize("flags, word", [(("--discriminator", "vgg"), "--discriminator"),
                                          (("--gan_type", "vanilla"), "--gan_type"), (("--unet_feat", "8"), "--unet_feat")])
@pytest.mark.parametrize("model", ["SRGAN", "EDSR"])
def test_cli_refuses_the_flags_with_another_model(tmp_path, capsys, model, flags, word):
    with pytest.raises(SystemExit):
        _parse(tmp_path, *flags, base=["--model_name", model, "--synthetic"])
    err = capsys.readouterr().err
    assert word in err and model in err


def test_trainer_refusals_name_the_flag():
    from pytorch_super_resolution_model_collection_amd import sr_trainers as T
    ns = lambda **kw: argparse.Namespace(**kw)
    assert T.check_discriminator_args(ns(crop_size=128), "esrgan") == ("vgg", "ragan", 64)
    assert T.check_discriminator_args(ns(discriminator="unet", crop_size=128), "esrgan") == ("unet", "vanilla", 64)
    assert T.check_discriminator_args(ns(discriminator="unet", unet_feat=16, crop_size=40), "esrgan") == ("unet", "vanilla", 16)
    assert T.check_discriminator_args(ns(), "edsr") is None
    for kw, word in ((dict(discriminator="unet", gan_type="ragan"), "gan_type"),
                     (dict(discriminator="unet", crop_size=36), "crop_size"), (dict(unet_feat=16), "unet_feat"),
                     (dict(discriminator="resnet"), "discriminator"), (dict(gan_type="lsgan"), "gan_type")):
        with pytest.raises(ValueError, match=word):
            T.check_discriminator_args(ns(**kw), "esrgan")
    for kw, word in ((dict(discriminator="vgg"), "discriminator"), (dict(gan_type="ragan"), "gan_type"),
                     (dict(unet_feat=64), "unet_feat")):
        for kind in ("srgan", "edsr"):
            with pytest.raises(ValueError, match=word):
                T.check_discriminator_args(ns(**kw), kind)
    pkg = _pkg()
    assert T.discriminator_kind(pkg.UNetDiscriminatorSN(3, 4).state_dict()) == "unet"
    assert T.discriminator_kind(pkg.ESRGANDiscriminator(3, 4, 16).state_dict()) == "vgg"


def test_step_refusals_name_the_argument():
    pkg = _pkg()
    D = pkg.UNetDiscriminatorSN(3, 4)
    with pytest.raises(ValueError, match="gan_type"):
        pkg.trainers.esrgan_segments(None, D, None, None, object(), gan_type="ragan")
    with pytest.raises(ValueError, match="gan_type"):
        pkg.trainers.esrgan_segments(None, D, None, None, object(), gan_type="lsgan")
    assert len(pkg.trainers.esrgan_segments(None, D, None, None, object(), gan_type="vanilla")) == 2
