"""The relativistic average GAN loss without a GPU: the host twin (srk_ragan_loss_host, the kernel's own header in double)
against fp64 autograd over the case table of tests/esrgan_ref.py, the edge cases, the refusals and the exported symbols."""
import ctypes

import pytest
import torch

import esrgan_ref as E

# both sides are fp64 and B <= 257: the two differ by summation order only
TOL = 1e-9


def _pkg():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _pkg()._lib.load()


def _host(lib, real, fake, for_generator, scale=1.0, want_real=True, want_fake=True):
    b = real.numel()
    loss = ctypes.c_double(float("nan"))
    dr = torch.full((b,), float("nan"), dtype=torch.float64) if want_real else None
    df = torch.full((b,), float("nan"), dtype=torch.float64) if want_fake else None
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = lib.srk_ragan_loss_host(p(real), p(fake), b, int(for_generator), scale, ctypes.byref(loss), p(dr), p(df))
    return rc, loss.value, dr, df


def _close(got, want):
    return float((got - want).abs().max()) <= TOL * max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize("for_generator", [False, True])
@pytest.mark.parametrize("name", sorted(E.RAGAN_CASES))
def test_host_twin_matches_autograd(lib, name, for_generator):
    real, fake = E.RAGAN_CASES[name]
    want, wr, wf = E.ragan_grads(real, fake, for_generator)
    rc, loss, dr, df = _host(lib, real, fake, for_generator)
    assert rc == 0
    assert loss == loss and abs(loss - float(want)) <= TOL * abs(float(want))
    assert torch.isfinite(dr).all() and torch.isfinite(df).all()
    assert _close(dr, wr) and _close(df, wf)
    # the seed scales both rows and leaves the loss alone
    rc, loss2, dr2, df2 = _host(lib, real, fake, for_generator, scale=0.005)
    assert rc == 0 and loss2 == loss
    assert _close(dr2, 0.005 * wr) and _close(df2, 0.005 * wf)


@pytest.mark.parametrize("for_generator", [False, True])
def test_extreme_logits_stay_finite_and_saturate(lib, for_generator):
    """A pair of logits 120 apart: softplus is the positive argument itself (no overflow), the other is ~0."""
    real, fake = torch.tensor([60.0, 60.0]), torch.tensor([-60.0, -60.0])
    rc, loss, dr, df = _host(lib, real, fake, for_generator)
    assert rc == 0
    # a = 120, b = -120: D: sp(-120) + sp(-120) ~ 0; G: sp(120) + sp(120) = 240, the mean over both rows 120
    assert abs(loss - (120.0 if for_generator else 0.0)) <= 1e-12 * 120.0 + 1e-50
    assert torch.isfinite(dr).all() and torch.isfinite(df).all()


def test_equal_rows(lib):
    """real == fake: a = b = real - mean, so both modes sum the same terms, and the generator's dL/da is the
    discriminator's dL/db and the other way round: the two modes' gradient rows are each other's, swapped."""
    real, fake = E.RAGAN_CASES["B16_equal"]
    _, ld, drd, dfd = _host(lib, real, fake, False)
    _, lg, drg, dfg = _host(lib, real, fake, True)
    assert abs(ld - lg) <= 1e-15
    assert _close(drg, dfd) and _close(dfg, drd)


@pytest.mark.parametrize("for_generator", [False, True])
def test_batch_of_one(lib, for_generator):
    """B = 1: a = r - f, b = f - r, and the loss is softplus(-+(r - f))."""
    real, fake = torch.tensor([0.75]), torch.tensor([-0.5])
    rc, loss, dr, df = _host(lib, real, fake, for_generator)
    x = torch.tensor(1.25, dtype=torch.float64)
    want = torch.nn.functional.softplus(x if for_generator else -x)
    assert rc == 0 and abs(loss - float(want)) <= 1e-14
    sig = float(torch.sigmoid(x if for_generator else -x))
    sign = 1.0 if for_generator else -1.0
    assert abs(float(dr[0]) - sign * sig) <= 1e-14 and abs(float(df[0]) + sign * sig) <= 1e-14


@pytest.mark.parametrize("for_generator", [False, True])
def test_a_null_gradient_row_is_skipped(lib, for_generator):
    real, fake = E.RAGAN_CASES["B3"]
    _, loss, dr, df = _host(lib, real, fake, for_generator)
    rc, loss2, none, df2 = _host(lib, real, fake, for_generator, want_real=False)
    assert rc == 0 and none is None and loss2 == loss and torch.equal(df2, df)
    rc, loss3, dr3, none = _host(lib, real, fake, for_generator, want_fake=False)
    assert rc == 0 and none is None and loss3 == loss and torch.equal(dr3, dr)


def test_bad_arguments_are_refused(lib):
    one = torch.zeros(4)
    p = ctypes.c_void_p(one.data_ptr())
    loss = ctypes.c_double()
    assert lib.srk_ragan_loss_host(p, p, 0, 0, 1.0, ctypes.byref(loss), None, None) == -1
    assert "B = 0" in lib.srk_last_error_string().decode()
    assert lib.srk_ragan_loss_host(p, p, -3, 1, 1.0, ctypes.byref(loss), None, None) == -1
    assert lib.srk_ragan_loss_host(None, p, 4, 0, 1.0, ctypes.byref(loss), None, None) == -1
    assert lib.srk_ragan_loss_host(p, None, 4, 0, 1.0, ctypes.byref(loss), None, None) == -1
    assert lib.srk_ragan_loss_host(p, p, 4, 0, 1.0, None, None, None) == -1
    # the device entry point refuses the same before it launches anything
    assert lib.srk_ragan_loss_forward_backward(p, p, 0, 0, 1.0, p, None, None, None, None) == -1
    assert lib.srk_ragan_loss_forward_backward(None, p, 4, 0, 1.0, p, None, None, None, None) == -1


def test_symbols_are_declared_and_exported(lib):
    L = _pkg()._lib
    declared = L.header_symbols()
    for n in ("srk_ragan_loss_forward_backward", "srk_ragan_loss_host"):
        assert n in declared and n in L._PROTOTYPES and hasattr(lib, n), n
    assert lib.srk_version() == 600
    assert callable(_pkg().ops.ragan_loss)
