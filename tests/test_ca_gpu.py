"""Channel attention on the GPU: ops.channel_attention (csrc/ca.hip) against the fp64 restatement of tests/ca_ref.py over
the issue's case table, in every input form ops accepts; run-to-run bits; the host twin; the skip's gradient; the exact
zeros of the saturated and the dead-hidden case.

The bars are the project's standing contracts, relative to the reference tensor's maximum: outputs 1e-4, gradients 1e-3.
Measured worst cases (profiles/ca_parity.txt) sit orders of magnitude inside; the bars stay where they are."""
import ctypes

import pytest
import torch

import ca_ref as R

pytestmark = pytest.mark.gpu

TOL_OUT, TOL_GRAD = 1e-4, 1e-3
FORMS = ("channels_last", "nchw", "sliced")


def _ops():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg.ops


_WANT = {}


def _want(name, skip):
    """The fp64 reference of a case, computed once and shared."""
    key = (name, skip)
    if key not in _WANT:
        case = R.make(name, skip)
        _WANT[key] = (case, R.restate(case))
    return _WANT[key]


def _form(v, form, gpu):
    """The same NCHW values on the device, behind the strides of `form`."""
    if v is None:
        return None
    if form == "channels_last":
        return v.to(gpu).contiguous(memory_format=torch.channels_last)
    if form == "nchw":
        return v.to(gpu).contiguous()
    n, c, h, w = v.shape      # a crop of a larger tensor: neither dense layout
    big = torch.zeros(n + 1, c, h + 3, w + 5)
    big[1:, :, 2:2 + h, 4:4 + w] = v
    return big.to(gpu)[1:, :, 2:2 + h, 4:4 + w]


def _run(case, gpu, form="channels_last", g_form=None):
    """ops.channel_attention forward and backward -> (y, dt, dx, dw1, db1, dw2, db2) on the device."""
    ops = _ops()
    t = _form(case.t, form, gpu).requires_grad_(True)
    x = _form(case.x, form, gpu)
    if x is not None:
        x.requires_grad_(True)
    par = [p.to(gpu).requires_grad_(True) for p in (case.w1, case.b1, case.w2, case.b2)]
    y = ops.channel_attention(t, x, *par)
    grads = torch.autograd.grad(y, [t] + ([x] if x is not None else []) + par, _form(case.g, g_form or form, gpu))
    dx = grads[1] if x is not None else None
    return (y.detach(), grads[0], dx) + tuple(grads[-4:])


def _check(got, want, case, what):
    y, dt, dx, dw1, db1, dw2, db2 = got
    worst = {}
    for name, a, b, tol in (("y", y, want.y, TOL_OUT), ("dt", dt, want.dt, TOL_GRAD), ("dw1", dw1, want.dw1, TOL_GRAD),
                            ("db1", db1, want.db1, TOL_GRAD), ("dw2", dw2, want.dw2, TOL_GRAD),
                            ("db2", db2, want.db2, TOL_GRAD)):
        assert tuple(a.shape) == tuple(b.shape), (what, name, tuple(a.shape))
        if float(b.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0, (what, name)     # (the dead-hidden case's exact zeros)
            continue
        worst[name] = R.worst(a, b)
        assert worst[name] <= tol, (what, name, worst[name])
    print("channel_attention %-28s " % what + "  ".join("%s %.2e" % kv for kv in worst.items()))
    if case.x is not None:
        assert torch.equal(dx.cpu(), case.g), what               # dL/dx is g


@pytest.mark.parametrize("skip", (False, True))
@pytest.mark.parametrize("name", R.cases())
def test_op_matches_fp64_restatement(gpu, name, skip):
    case, want = _want(name, skip)
    _check(_run(case, gpu), want, case, "%s skip %d" % (name, skip))


@pytest.mark.parametrize("form", FORMS[1:])
@pytest.mark.parametrize("name", ("scalar", "net_odd", "mid"))
def test_input_forms(gpu, name, form):
    """NCHW-contiguous and sliced-view inputs give the bits of the channels_last call."""
    case, want = _want(name, True)
    base = _run(case, gpu)
    got = _run(case, gpu, form)
    _check(got, want, case, "%s %s" % (name, form))
    for a, b in zip(got, base):
        assert torch.equal(a, b), (name, form)
    assert got[0].permute(0, 2, 3, 1).is_contiguous()            # y is channels_last, as every activation here


@pytest.mark.parametrize("name", ("scalar", "net_odd", "wide", "patch"))
def test_two_calls_give_the_same_bits(gpu, name):
    case, _ = _want(name, True)
    first, again = _run(case, gpu), _run(case, gpu)
    for what, a, b in zip(("y", "dt", "dx", "dw1", "db1", "dw2", "db2"), first, again):
        assert torch.equal(a, b), (name, what)


@pytest.mark.parametrize("name", ("hw1", "scalar", "net_odd", "patch"))
def test_device_matches_host_twin(gpu, name):
    """The kernels and srk_channel_attention_host compile one MLP; the device rounds m, h, s, y and dt to fp32."""
    import pytorch_super_resolution_model_collection_amd as pkg
    case, _ = _want(name, True)
    twin = R.host(pkg._lib.load(), case)
    y, dt, dx, dw1, db1, dw2, db2 = _run(case, gpu)
    for what, a, b in (("y", y, twin.y), ("dt", dt, twin.dt), ("dw1", dw1, twin.dw1), ("db1", db1, twin.db1),
                       ("dw2", dw2, twin.dw2), ("db2", db2, twin.db2)):
        # one fp32 rounding of the result and of each of m, h, s behind it: 2^-24 each, times the MLP's gain; 1e-5 is
        # far above that and far below the contract
        assert R.worst(a, b) <= 1e-5, (name, what, R.worst(a, b))


def test_skip_gradient_is_g_itself(gpu):
    """Autograd hands the skip the very tensor it handed the op: no kernel, no copy."""
    ops = _ops()
    case, _ = _want("mid", True)
    t = _form(case.t, "channels_last", gpu).requires_grad_(True)
    x = _form(case.x, "channels_last", gpu).requires_grad_(True)
    par = [p.to(gpu) for p in (case.w1, case.b1, case.w2, case.b2)]
    g = _form(case.g, "channels_last", gpu)
    seen = []
    x.register_hook(lambda gr: seen.append(gr.data_ptr()))
    ops.channel_attention(t, x, *par).backward(g)
    assert seen == [g.data_ptr()]
    assert torch.equal(x.grad, g)
    with torch.no_grad():                                       # no graph: nothing saved, the same y
        y = ops.channel_attention(t, x, *par)
    assert torch.equal(y, ops.channel_attention(t, x, *par).detach())


def _raw(case, gpu):
    """The C entry points themselves -> (y, m, h, s, dt, dw1, db1, dw2, db2), for what the autograd function keeps to
    itself (the saved gate)."""
    import pytorch_super_resolution_model_collection_amd as pkg
    lib = pkg._lib.load()
    n, c, hh, ww = case.t.shape
    cr = case.w1.shape[0]
    cl = lambda v: v.to(gpu).contiguous(memory_format=torch.channels_last)
    t, g = cl(case.t), cl(case.g)
    w1, b1, w2, b2 = (p.to(gpu).contiguous() for p in (case.w1, case.b1, case.w2, case.b2))
    new = lambda *shape: torch.full(shape, float("nan"), device=gpu)
    y, dt, m, h, s = torch.empty_like(t), torch.empty_like(t), new(n, c), new(n, cr), new(n, c)
    dw1, db1, dw2, db2 = new(cr, c), new(cr), new(c, cr), new(c)
    nbytes = lib.srk_channel_attention_workspace(n, hh, ww, c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.srk_channel_attention_forward(p(t), None, p(w1), p(b1), p(w2), p(b2), n, hh, ww, c, cr, p(y), p(m), p(h), p(s),
                                             p(ws), nbytes, st) == 0, lib.srk_last_error_string()
    assert lib.srk_channel_attention_backward(p(g), p(t), p(w1), p(w2), p(m), p(h), p(s), n, hh, ww, c, cr, p(dt), p(dw1),
                                              p(db1), p(dw2), p(db2), 0.0, p(ws), nbytes, st) == 0, lib.srk_last_error_string()
    torch.cuda.synchronize()
    return t, g, y, m, h, s, dt, dw1, db1, dw2, db2


def test_saturated_gate(gpu):
    """b2 = +40: s = 1 exactly, s (1 - s) = 0, nothing flows back through those channels' gates and dt = g there, bit for
    bit.  b2 = -40: s = sigmoid(-40 + W2 h) ~ 4e-18 is a normal fp32 number, so s (1 - s) = s, not an exact zero: there
    dt = g * s + dm / HW is held to its size (|W2 h| <= 10: s < 1e-13; see tests/test_ca_cpu.py)."""
    case, _ = _want("saturated", False)
    t, g, y, m, h, s, dt, dw1, db1, dw2, db2 = _raw(case, gpu)
    half = case.t.shape[1] // 2
    assert bool((s[:, :half] == 1.0).all()) and float(s[:, half:].max()) < 1e-13
    assert torch.equal(y[:, :half], t[:, :half]) and torch.equal(dt[:, :half], g[:, :half])
    assert float(db2[:half].abs().max()) == 0.0 and float(dw2[:half].abs().max()) == 0.0
    assert float(dt[:, half:].abs().max()) < 1e-9


def test_dead_hidden_layer(gpu):
    """b1 = -1e3: h = 0, so dh = 0, dm = 0, dW1 = db1 = 0 and dW2 = 0 exactly, and dt = g * s."""
    case, _ = _want("dead_hidden", False)
    t, g, y, m, h, s, dt, dw1, db1, dw2, db2 = _raw(case, gpu)
    for what, v in (("h", h), ("dw1", dw1), ("db1", db1), ("dw2", dw2)):
        assert float(v.abs().max()) == 0.0, what
    assert torch.equal(dt, g * s[:, :, None, None])
    assert float(db2.abs().max()) > 0.0


def test_accumulating_parameter_gradients(gpu):
    """beta = 1, what optim.FlatParams' buffers get: out = out + gradient; NULL outputs are left alone."""
    import pytorch_super_resolution_model_collection_amd as pkg
    ops = _ops()
    case, want = _want("mid", True)
    t, x = (_form(v, "channels_last", gpu).requires_grad_(True) for v in (case.t, case.x))
    par = [torch.nn.Parameter(p.to(gpu)) for p in (case.w1, case.b1, case.w2, case.b2)]
    for p in par:
        p._srk_grad = torch.ones_like(p)
    y = ops.channel_attention(t, x, *par)
    y.backward(_form(case.g, "channels_last", gpu))
    for p, ref in zip(par, (want.dw1, want.db1, want.dw2, want.db2)):
        assert p.grad is None                                    # accumulated in place, nothing handed to autograd
        assert R.worst(p._srk_grad - 1.0, ref) <= TOL_GRAD
