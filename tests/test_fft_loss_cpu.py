"""The frequency-domain loss without a GPU: the restatement (tests/fft_loss_ref.py) against torch.fft.fft2, fp64 autograd
and central differences; srk_fft_loss_host (the kernels' definition in plain C++ double: same table, same arithmetic
header, csrc/fft_loss_common.h) against the restatement on the case table; the exact entries of srk_dft_table_host; the
argument checks of both entry points; trainers.mixed_loss's identities and --fft_weight.  The device kernels are held to
the same table in tests/test_fft_loss_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import fft_loss_ref as L

LOSS_RTOL = 1e-12          # both sides are fp64; only the summation order differs
GRAD_RTOL, GRAD_ATOL = 1e-10, 1e-15
SIGN_GUARD = 1e-9          # no free bin may be closer to zero than this times max |F|


@pytest.fixture(scope="module")
def lib():
    return L._lib()


def host_loss(lib, pred, gt, norm="backward", grad_scale=1.0, want_grad=True, strides=True):
    """pred, gt: fp32 numpy views [N,C,H,W] of any strides -> (loss, gradient as fp64 [N,C,H,W] or None)."""
    n, c, h, w = pred.shape
    p = np.ascontiguousarray(pred.transpose(0, 2, 3, 1))          # NHWC dense, as the entry point takes pred
    d = np.full((n, h, w, c), np.nan, np.float64) if want_grad else None
    st = (ctypes.c_int64 * 4)(*[s // 4 for s in gt.strides]) if strides else None
    loss = ctypes.c_double(-1.0)
    rc = lib.srk_fft_loss_host(ctypes.c_void_p(p.ctypes.data), ctypes.c_void_p(gt.ctypes.data), st, n, c, h, w,
                               L.norm_scale(norm, h, w), grad_scale, ctypes.byref(loss),
                               ctypes.c_void_p(d.ctypes.data) if want_grad else None)
    assert rc == 0, lib.srk_last_error_string()
    return loss.value, (d.transpose(0, 3, 1, 2) if want_grad else None)


def laid_out(a, layout):
    if layout == 'nchw':
        return np.ascontiguousarray(a)
    if layout == 'channels_last':
        return np.ascontiguousarray(a.transpose(0, 2, 3, 1)).transpose(0, 3, 1, 2)
    big = np.full((a.shape[0], a.shape[1], a.shape[2] + 5, a.shape[3] + 9), 7.0, np.float32)   # a crop of a larger tensor
    big[:, :, 2:2 + a.shape[2], 6:6 + a.shape[3]] = a
    return big[:, :, 2:2 + a.shape[2], 6:6 + a.shape[3]]


def test_table_entries(lib):
    """Exactly 0 and +-1 wherever 4k is a multiple of n, entry n - k the conjugate of entry k, nothing else exact."""
    for n in (1, 2, 4, 8, 12, 7):
        t = L.table(n)
        for k in range(n):
            want = np.array([np.cos(2 * np.pi * k / n), np.sin(2 * np.pi * k / n)])
            assert np.abs(t[k] - want).max() <= 1e-15, (n, k)
            if (4 * k) % n == 0:
                q = 4 * k // n
                assert tuple(t[k]) == ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[q], (n, k, t[k])
            else:
                assert not np.isin(t[k], (0.0, 1.0, -1.0)).any(), (n, k, t[k])
            if k:
                assert t[n - k][0] == t[k][0] and t[n - k][1] == -t[k][1], (n, k)
    assert [k for k in range(7) if np.isin(L.table(7)[k], (0.0, 1.0, -1.0)).any()] == [0]   # n = 7: only the unit itself
    assert tuple(L.table(12)[3]) == (0.0, 1.0) and tuple(L.table(8)[6]) == (0.0, -1.0)
    assert lib.srk_dft_table_host(0, L.table(4).ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1
    assert lib.srk_dft_table_host(4, None) == -1


@pytest.mark.parametrize("name", sorted(L.cases()))
def test_the_restatement_itself(name):
    """The spectrum against torch.fft.fft2 in fp64, the sign guard, the closed-form gradient against autograd through the
    same matrices and against a central difference at three pixels."""
    p, g, norm = L.cases()[name]
    d = p.astype(np.float64) - g.astype(np.float64)
    fre, fim = L.spectrum(d, norm)
    lib_f = torch.fft.fft2(torch.from_numpy(d), norm=norm).numpy()
    top = max(np.abs(lib_f).max(), 1e-300)
    assert np.abs(fre - lib_f.real).max() <= 1e-12 * top and np.abs(fim - lib_f.imag).max() <= 1e-12 * top

    low, top = L.sign_margin(name)                      # on the reference alone; no case skipped, no bin masked
    print("%-22s smallest free |Re F|, |Im F| = %.3e = %.2e of max |F| %.3e" % (name, low, low / top if top else 0.0, top))
    if name == "identical":
        assert low == 0.0 and top == 0.0                # every bin is an exact zero: the sign is 0 everywhere
    else:
        assert low >= SIGN_GUARD * top, (name, low, top)

    want_loss, want_grad = L.reference(name)
    x = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
    loss = L.torch_loss(x, torch.from_numpy(g.astype(np.float64)), norm)
    loss.backward()
    assert abs(float(loss.detach()) - want_loss) <= 1e-13 * max(1.0, abs(want_loss))
    assert np.abs(x.grad.numpy() - want_grad).max() <= 1e-13 * max(np.abs(want_grad).max(), 1e-300)
    if name == "identical":
        assert want_loss == 0.0 and not want_grad.any()
        return
    n, c, h, w = p.shape
    for (r, q) in ((0, 0), (h // 2, w // 3), (h - 1, w - 1)):
        # |F| is piecewise linear in a pixel: the step keeps every free bin (>= low) on its side of zero
        e = 0.25 * low / L.norm_scale(norm, h, w)
        hi, lo = p.astype(np.float64), p.astype(np.float64)
        hi[-1, -1, r, q] += e
        lo[-1, -1, r, q] -= e
        f = lambda a: float(L.torch_loss(torch.from_numpy(a), torch.from_numpy(g.astype(np.float64)), norm))
        num = (f(hi) - f(lo)) / (2 * e)
        assert abs(num - want_grad[-1, -1, r, q]) <= 1e-5 * np.abs(want_grad).max() + 1e-13 * want_loss / e, (name, r, q, num)


@pytest.mark.parametrize("name", [n for n in sorted(L.cases()) if n not in L.DEVICE_ONLY])
def test_host_twin_matches_the_restatement(lib, name):
    p, g, norm = L.cases()[name]
    want_loss, want_grad = L.reference(name)
    loss, grad = host_loss(lib, p, g, norm)
    bar = GRAD_RTOL * np.abs(want_grad).max() + GRAD_ATOL
    err = np.abs(grad - want_grad).max()
    print("srk_fft_loss_host %-22s loss %.15f (restated %.15f)  worst |d grad| %.3g (bar %.3g)"
          % (name, loss, want_loss, err, bar))
    assert abs(loss - want_loss) <= LOSS_RTOL * max(1.0, abs(want_loss)), (name, loss, want_loss)
    assert err <= bar, (name, err, bar)
    if name == "identical":
        assert loss == 0.0 and not grad.any()
    if name == "out_of_range":     # nothing clamps the prediction
        assert ((p < 0) | (p > 1)).sum() > 50 and abs(loss) > 0.1


@pytest.mark.parametrize("layout", ("nchw", "channels_last", "cropped_view"))
def test_target_strides_scale_and_loss_only(lib, layout):
    p, g, norm = L.cases()["05_2x3x7x5"]
    loss, grad = host_loss(lib, p, g)
    loss2, grad2 = host_loss(lib, p, laid_out(g, layout), grad_scale=0.25)
    assert loss2 == loss and np.abs(grad2 - 0.25 * grad).max() <= 1e-15 * np.abs(grad).max()
    assert np.array_equal(host_loss(lib, p, laid_out(g, layout))[1], grad)       # the layouts give the same bits
    assert host_loss(lib, p, g, want_grad=False) == (loss, None)
    if layout == 'channels_last':   # NULL strides: the target NHWC-dense
        assert host_loss(lib, p, laid_out(g, layout), strides=False)[0] == loss


def test_a_nan_stays_in_its_plane(lib):
    p, g, norm = [a.copy() if isinstance(a, np.ndarray) else a for a in L.cases()["05_2x3x7x5"]]
    p[1, 2, 3, 4] = np.nan
    loss, grad = host_loss(lib, p, g)
    assert np.isnan(loss) and np.isnan(grad[1, 2]).all()
    grad[1, 2] = 0
    assert np.isfinite(grad).all()


def test_argument_checks(lib):
    buf = np.zeros(4 * 3 * 32 * 32, np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)
    out = ctypes.c_double(0.0)
    assert lib.srk_fft_loss_workspace_bytes(1, 3, 32, 32) >= 8 + 2 * 3 * 32 * 17 * 16
    assert lib.srk_fft_loss_workspace_bytes(1, 3, 257, 32) == 0 and lib.srk_fft_loss_workspace_bytes(0, 3, 32, 32) == 0
    dev = lambda *a, **k: lib.srk_fft_loss_forward_backward(a[0], a[1], None, a[2], a[3], a[4], a[5], k.get("tables", p),
                                                            k.get("scale", 1.0), 1.0, a[6], None, a[7], None)
    host = lambda *a, **k: lib.srk_fft_loss_host(a[0], a[1], None, a[2], a[3], a[4], a[5], k.get("scale", 1.0), 1.0,
                                                 ctypes.byref(out), None)
    for call in (dev, host):   # (all refused before anything is launched or read: no device is needed)
        assert call(p, p, 1, 3, 257, 32, p, p) == -2 and b"256" in lib.srk_last_error_string()
        assert call(p, p, 1, 3, 32, 257, p, p) == -2 and b"32 x 257" in lib.srk_last_error_string()
        assert call(p, p, 1, 3, 0, 32, p, p) == -1
        assert call(p, p, 0, 3, 32, 32, p, p) == -1
        assert call(p, p, 1, -3, 32, 32, p, p) == -1
        assert call(None, p, 1, 3, 32, 32, p, p) == -1
        assert call(p, None, 1, 3, 32, 32, p, p) == -1
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            assert call(p, p, 1, 3, 32, 32, p, p, scale=bad) == -1
    assert dev(p, p, 1, 3, 32, 32, None, p) == -1                 # no loss
    assert dev(p, p, 1, 3, 32, 32, p, None) == -1                 # no workspace
    assert dev(p, p, 1, 3, 32, 32, p, p, tables=None) == -1       # no tables
    assert lib.srk_version() == 600


def test_mixed_loss_identities():
    import pytorch_super_resolution_model_collection_amd as pkg
    T, ops = pkg.trainers, pkg.ops
    for pixel in (ops.mse_loss, ops.l1_loss, ops.charbonnier_loss):
        assert T.mixed_loss(pixel) is pixel
        assert T.mixed_loss(pixel, 0.0, 0.0) is pixel and T.mixed_loss(pixel, ssim_weight=0.0, fft_weight=0.0, fft_norm="ortho") is pixel
        assert T.mixed_loss(pixel, 0.0, 0.1) is not pixel
    # w == 0: what it returns today -- the two-term closure over the same pixel loss and weight
    today, kept = T.mixed_loss(ops.l1_loss, 0.3), T.mixed_loss(ops.l1_loss, 0.3, 0.0, "ortho")
    assert today.__code__ is kept.__code__ and today.__code__ is not T.mixed_loss(ops.l1_loss, 0.3, 0.1).__code__
    cells = lambda f: [c.cell_contents for c in f.__closure__]
    assert cells(today) == cells(kept) and ops.l1_loss in cells(today) and 0.3 in cells(today)
    for bad in (dict(fft_weight=-0.1), dict(fft_weight=float('nan')), dict(fft_weight=float('inf')), dict(fft_weight=0.1, fft_norm="forward"),
                dict(ssim_weight=1.5, fft_weight=0.1)):
        with pytest.raises(ValueError):
            T.mixed_loss(ops.l1_loss, **bad)
    with pytest.raises(ValueError):
        ops.fft_loss(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4), norm="forward")
    with pytest.raises(ValueError):
        pkg.utils.FFTLoss(norm="forward")
    assert pkg.utils.FFTLoss("ortho").norm == "ortho"


@pytest.mark.parametrize("a", (0.0, 0.3))
@pytest.mark.parametrize("w", (0.0, 0.25))
@pytest.mark.parametrize("v", (0.0, 2.0))
def test_mixed_loss_is_the_ssim_mix_inside_fft_inside_lpips(monkeypatch, a, w, v):
    """The call tree of one evaluation of the loss, recorded: pred is forked once per stage, the SSIM mix weighs its two
    terms (1 - a, a), every additive stage is loss_sum(inner(p1), weighted_term(term, weight, p2), 1.0, weight), FFT around
    the mix and LPIPS outermost."""
    import pytorch_super_resolution_model_collection_amd as pkg
    T, ops = pkg.trainers, pkg.ops
    forks, net = [], object()

    def fork(x):
        forks.append(x)
        return (x, 1), (x, 2)
    monkeypatch.setattr(ops, "fork", fork)
    monkeypatch.setattr(ops, "loss_sum", lambda l1, l2, ca=1.0, cb=1.0: ("sum", l1, l2, ca, cb))
    monkeypatch.setattr(ops, "weighted_term", lambda fn, weight, p, t: ("term", fn(p, t), weight))
    monkeypatch.setattr(ops, "ssim_loss", lambda p, t: ("ssim", p, t))
    monkeypatch.setattr(ops, "fft_loss", lambda p, t, norm: ("fft", p, t, norm))
    monkeypatch.setattr(ops, "lpips", lambda p, t, n, normalize=False: ("lpips", p, t, n, normalize))
    pixel = lambda p, t: ("pixel", p, t)
    loss = T.mixed_loss(pixel, a, w, "ortho", v, net)
    if a == w == v == 0.0:
        assert loss is pixel
        return

    def mix(p):
        if a == 0.0:
            return ("pixel", p, "t")
        return ("sum", ("term", ("pixel", (p, 1), "t"), 1.0 - a), ("term", ("ssim", (p, 2), "t"), a), 1.0 - a, a)

    def with_fft(p):
        if w == 0.0:
            return mix(p)
        return ("sum", mix((p, 1)), ("term", ("fft", (p, 2), "t", "ortho"), w), 1.0, w)

    def with_lpips(p):
        if v == 0.0:
            return with_fft(p)
        return ("sum", with_fft((p, 1)), ("term", ("lpips", (p, 2), "t", net, True), v), 1.0, v)
    assert loss("x", "t") == with_lpips("x")
    assert len(forks) == (a > 0) + (w > 0) + (v > 0)
    if a > 0 and w > 0 and v > 0:      # all three, written out
        assert forks == ["x", ("x", 1), (("x", 1), 1)]
        assert loss("x", "t") == (
            "sum",
            ("sum",
             ("sum", ("term", ("pixel", ((("x", 1), 1), 1), "t"), 1.0 - 0.3), ("term", ("ssim", ((("x", 1), 1), 2), "t"), 0.3),
              1.0 - 0.3, 0.3),
             ("term", ("fft", (("x", 1), 2), "t", "ortho"), 0.25), 1.0, 0.25),
            ("term", ("lpips", ("x", 2), "t", net, True), 2.0), 1.0, 2.0)


def test_trainers_refuse_srgan_and_drcn():
    import argparse
    from pytorch_super_resolution_model_collection_amd import sr_trainers
    for cls in (sr_trainers.SRGAN, sr_trainers.DRCN):
        with pytest.raises(ValueError, match="fft_weight"):
            cls(argparse.Namespace(model_name=cls.__name__, fft_weight=0.1))


def test_cli_fft_weight(tmp_path, capsys):
    import main
    base = ['--save_dir', str(tmp_path / "r")]
    a = main.parse_args(base + ['--model_name', 'EDSR'])
    assert a.fft_weight == 0.0 and a.fft_norm == 'backward'
    a = main.parse_args(base + ['--model_name', 'EDSR', '--fft_weight', '0.05', '--fft_norm', 'ortho'])
    assert a.fft_weight == 0.05 and a.fft_norm == 'ortho'
    assert main.parse_args(base + ['--model_name', 'LapSRN', '--fft_weight', '2', '--crop_size', '256']).fft_weight == 2.0
    assert main.parse_args(base + ['--model_name', 'SRGAN', '--fft_weight', '0']).fft_weight == 0.0
    assert main.parse_args(base + ['--model_name', 'EDSR', '--crop_size', '384']).crop_size == 384    # no term, no limit
    # --synthetic: allowed, as with --ssim_weight
    assert main.parse_args(base + ['--model_name', 'ESPCN', '--synthetic', '--fft_weight', '0.1']).synthetic
    for bad in ('-0.1', 'nan', 'inf', 'much'):
        with pytest.raises(SystemExit):
            main.parse_args(base + ['--model_name', 'EDSR', '--fft_weight=' + bad])
        assert '--fft_weight' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main.parse_args(base + ['--model_name', 'EDSR', '--fft_weight', '0.1', '--fft_norm', 'forward'])
    assert '--fft_norm' in capsys.readouterr().err
    for model in ('SRGAN', 'DRCN'):
        with pytest.raises(SystemExit):
            main.parse_args(['--save_dir', str(tmp_path / model), '--model_name', model, '--fft_weight', '0.1'])
        err = capsys.readouterr().err
        assert model in err and '--fft_weight' in err
        assert not (tmp_path / model).exists()      # refused at argument checking: nothing was set up
    with pytest.raises(SystemExit):
        main.parse_args(['--save_dir', str(tmp_path / "big"), '--model_name', 'EDSR', '--fft_weight', '0.1', '--crop_size', '257'])
    err = capsys.readouterr().err
    assert '256' in err and '--crop_size' in err and not (tmp_path / "big").exists()
