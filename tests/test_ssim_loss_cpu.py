"""The SSIM training loss without a GPU: srk_ssim_loss_host (the kernel's definition in plain C++ double: same window
table and formula header, csrc/ssim_common.h) against fp64 torch autograd (tests/ssim_loss_ref.py) on the SSIM case table,
the argument checks of both entry points, and --ssim_weight.  The device kernel is held to the same table in
tests/test_ssim_loss_gpu.py."""
import ctypes

import numpy as np
import pytest

import __graft_entry__
import ssim_loss_ref as L
import ssim_ref as R

LOSS_TOL = 1e-12          # both sides are fp64; only the summation order differs
GRAD_RTOL, GRAD_ATOL = 1e-10, 1e-15


@pytest.fixture(scope="module")
def lib():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    return p._lib.load()


def host_loss(lib, pred, gt, grad_scale=1.0, want_grad=True, strides=True):
    """pred, gt: fp32 numpy views [N,C,H,W] of any strides -> (loss, gradient as fp64 [N,C,H,W] or None)."""
    n, c, h, w = pred.shape
    p = np.ascontiguousarray(pred.transpose(0, 2, 3, 1))          # NHWC dense, as the entry point takes pred
    d = np.full((n, h, w, c), np.nan, np.float64) if want_grad else None
    st = (ctypes.c_int64 * 4)(*[s // 4 for s in gt.strides]) if strides else None
    loss = ctypes.c_double(-1.0)
    rc = lib.srk_ssim_loss_host(ctypes.c_void_p(p.ctypes.data), ctypes.c_void_p(gt.ctypes.data), st, n, c, h, w, grad_scale,
                                ctypes.byref(loss), ctypes.c_void_p(d.ctypes.data) if want_grad else None)
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


def test_the_restatement_itself():
    """Within [0, 1] the loss is 1 - the SSIM of ssim_ref; the autograd gradient agrees with a central difference."""
    p, g = L.cases()["picture"]
    loss, grad = L.loss_and_grad(p, g)
    assert abs(loss - (1 - R.ssim_map(p.astype(np.float64), g.astype(np.float64)).mean())) < 1e-14
    q = p.astype(np.float64)
    for (r, c) in ((0, 0), (40, 77), (96, 130)):
        e = 1e-6
        hi, lo = q.copy(), q.copy()
        hi[0, 0, r, c] += e
        lo[0, 0, r, c] -= e
        num = ((1 - R.ssim_map(hi, g.astype(np.float64)).mean()) - (1 - R.ssim_map(lo, g.astype(np.float64)).mean())) / (2 * e)
        assert abs(num - grad[0, 0, r, c]) < 1e-8 * max(1.0, abs(grad).max()), (r, c, num, grad[0, 0, r, c])


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_host_twin_matches_autograd(lib, name):
    p, g = L.cases()[name]
    want_loss, want_grad = L.reference(name)
    loss, grad = host_loss(lib, p, g)
    bar = GRAD_RTOL * np.abs(want_grad).max() + GRAD_ATOL
    err = np.abs(grad - want_grad).max()
    print("srk_ssim_loss_host %-14s loss %.15f (autograd %.15f)  worst |d grad| %.3g (bar %.3g)" % (name, loss, want_loss, err, bar))
    assert abs(loss - want_loss) <= LOSS_TOL, (name, loss, want_loss)
    assert err <= bar, (name, err, bar)
    if name == "identical":
        assert loss == 0.0 and np.abs(grad).max() < 1e-12
    if name == "batch_rgb":   # the prediction is read unclamped: pixels outside [0, 1] pull as hard as the others
        out = L.out_of_range(p)
        assert out.sum() > 100 and (grad[out] != 0).all() and (want_grad[out] != 0).all()


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_target_strides_scale_and_loss_only(lib, layout):
    p, g = L.cases()["batch_rgb"]
    loss, grad = host_loss(lib, p, g)
    loss2, grad2 = host_loss(lib, p, laid_out(g, layout), grad_scale=0.25)
    assert loss2 == loss and np.abs(grad2 - 0.25 * grad).max() <= 1e-15 * np.abs(grad).max()
    assert host_loss(lib, p, g, want_grad=False) == (loss, None)
    if layout == 'channels_last':   # NULL strides: the target NHWC-dense
        assert host_loss(lib, p, laid_out(g, layout), strides=False)[0] == loss


def test_a_nan_propagates(lib):
    p, g = [a.copy() for a in L.cases()["picture"]]
    p[0, 0, 50, 60] = np.nan
    loss, grad = host_loss(lib, p, g)
    assert np.isnan(loss) and np.isnan(grad[0, 0, 50, 60]) and np.isfinite(grad[0, 0, 10, 10])


def test_argument_checks(lib):
    buf = np.zeros(4 * 3 * 32 * 32, np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)
    out = ctypes.c_double(0.0)
    assert lib.srk_ssim_loss_workspace_bytes() >= 8
    dev = lambda *a: lib.srk_ssim_loss_forward_backward(a[0], a[1], None, a[2], a[3], a[4], a[5], 1.0, a[6], None, a[7], None)
    host = lambda *a: lib.srk_ssim_loss_host(a[0], a[1], None, a[2], a[3], a[4], a[5], 1.0, ctypes.byref(out), None)
    for call in (dev, host):   # (all refused before anything is launched or read)
        assert call(p, p, 1, 3, 10, 32, p, p) == -1 and b"10 x 32" in lib.srk_last_error_string()
        assert call(p, p, 1, 3, 32, 10, p, p) == -1
        assert call(p, p, 0, 3, 32, 32, p, p) == -1
        assert call(None, p, 1, 3, 32, 32, p, p) == -1
        assert call(p, None, 1, 3, 32, 32, p, p) == -1
    assert dev(p, p, 1, 3, 32, 32, None, p) == -1     # no loss
    assert dev(p, p, 1, 3, 32, 32, p, None) == -1     # no workspace
    assert lib.srk_version() == 600


def test_cli_ssim_weight(tmp_path, capsys):
    import main
    base = ['--save_dir', str(tmp_path / "r")]
    assert main.parse_args(base + ['--model_name', 'EDSR']).ssim_weight == 0.0
    assert main.parse_args(base + ['--model_name', 'EDSR', '--ssim_weight', '0.2']).ssim_weight == 0.2
    assert main.parse_args(base + ['--model_name', 'LapSRN', '--ssim_weight', '1']).ssim_weight == 1.0
    assert main.parse_args(base + ['--model_name', 'SRGAN', '--ssim_weight', '0']).ssim_weight == 0.0
    for bad in ('-0.1', '1.5', 'nan', 'inf', 'much'):
        with pytest.raises(SystemExit):
            main.parse_args(base + ['--model_name', 'EDSR', '--ssim_weight=' + bad])
        assert '--ssim_weight' in capsys.readouterr().err
    for model in ('SRGAN', 'DRCN'):
        with pytest.raises(SystemExit):
            main.parse_args(['--save_dir', str(tmp_path / model), '--model_name', model, '--ssim_weight', '0.2'])
        assert model in capsys.readouterr().err
        assert not (tmp_path / model).exists()      # refused at argument checking: nothing was set up
