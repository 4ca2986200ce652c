"""ops.window_attention on the GPU against the fp64 restatement of tests/swinir_ref.py, over the case table there: forward,
dqkv and dtable, repeated calls, the unshifted case against the unmasked restatement, a strided output gradient, and
the refusals.

Bars: the project's standing contracts -- values within 1e-4, gradients within 1e-3 of fp64, relative to the reference
tensor's maximum.  The fp32 FMA kernel sits in the 1e-6 range (profiles/swinir_parity.txt)."""
import pytest
import torch

import swinir_ref as R

pytestmark = pytest.mark.gpu

TOL_FWD, TOL_GRAD = 1e-4, 1e-3


def _ops():
    import pytorch_super_resolution_model_collection_amd as pkg
    return pkg.ops


@pytest.fixture(scope="module")
def refs():
    """The fp64 (out, dqkv, dtable) of every case, computed once and left unchanged."""
    return {name: R.attention_with_grads(case) for name, case in R.CASES.items()}


def _run(gpu, case, seed=0, dout=None):
    n, h, w, c, heads, window, shift = case
    qkv, table, g = R.inputs(case, seed)
    qkv = qkv.to(gpu).requires_grad_()
    table = table.to(gpu).requires_grad_()
    out = _ops().window_attention(qkv, table, heads, window, shift)
    out.backward(g.to(gpu) if dout is None else dout)
    return out.detach(), qkv.grad, table.grad


@pytest.mark.parametrize("name", list(R.CASES))
def test_matches_fp64(gpu, refs, name):
    out, dqkv, dtable = _run(gpu, R.CASES[name])
    want = refs[name]
    errs = [R.worst(a, b) for a, b in zip((out, dqkv, dtable), want)]
    print("window_attention %-16s out %.3e  dqkv %.3e  dtable %.3e of max |ref|" % ((name,) + tuple(errs)))
    assert errs[0] <= TOL_FWD and errs[1] <= TOL_GRAD and errs[2] <= TOL_GRAD, errs


@pytest.mark.parametrize("name", list(R.CASES))
def test_two_calls_are_bit_equal(gpu, name):
    a, b = _run(gpu, R.CASES[name]), _run(gpu, R.CASES[name])
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["one_window", "d30_classical"])
def test_no_shift_is_the_unmasked_restatement(gpu, name):
    n, h, w, c, heads, window, _ = R.CASES[name]
    case = (n, h, w, c, heads, window, 0)
    qkv, table, _ = R.inputs(case, 5)
    want = R.window_attention(qkv.double(), table.double(), heads, window, 0, masked=False)
    with torch.no_grad():      # the inference form: no log-sum-exp is written
        got = _ops().window_attention(qkv.to(gpu), table.to(gpu), heads, window, 0)
    assert R.worst(got, want) <= TOL_FWD


def test_a_mask_matters(gpu, refs):
    """The shifted case differs from the unmasked restatement by far more than the bar: the mask is applied."""
    n, h, w, c, heads, window, shift = case = R.CASES["2x3_windows"]
    qkv, table, _ = R.inputs(case, 0)
    unmasked = R.window_attention(qkv.double(), table.double(), heads, window, shift, masked=False)
    assert R.worst(unmasked, refs["2x3_windows"][0]) > 100 * TOL_FWD


def test_strided_output_gradient(gpu, refs):
    """A non-contiguous dO (a transposed buffer viewed back) is copied, never read with the wrong strides."""
    case = R.CASES["2x3_windows"]
    n, h, w, c = case[:4]
    g = R.inputs(case, 0)[2].to(gpu)
    strided = g.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not strided.is_contiguous() and torch.equal(strided, g)
    out, dqkv, dtable = _run(gpu, case, dout=strided)
    want = refs["2x3_windows"]
    assert R.worst(dqkv, want[1]) <= TOL_GRAD and R.worst(dtable, want[2]) <= TOL_GRAD


def test_refusals_name_the_number(gpu):
    ops = _ops()
    z = lambda *s: torch.zeros(*s, device=gpu)
    with pytest.raises(ValueError, match="window 9"):
        ops.window_attention(z(1, 9, 9, 12), z(289, 2), 2, 9, 0)
    with pytest.raises(ValueError, match="window 1"):
        ops.window_attention(z(1, 4, 4, 12), z(1, 2), 2, 1, 0)
    with pytest.raises(ValueError, match="shift 4"):
        ops.window_attention(z(1, 4, 4, 12), z(49, 2), 2, 4, 4)
    with pytest.raises(ValueError, match="6 x 8"):
        ops.window_attention(z(1, 6, 8, 12), z(49, 2), 2, 4, 0)
    with pytest.raises(ValueError, match="head dimension 33"):
        ops.window_attention(z(1, 4, 4, 99), z(49, 1), 1, 4, 0)
    with pytest.raises(ValueError, match="3 heads"):
        ops.window_attention(z(1, 4, 4, 12), z(49, 3), 3, 4, 0)
    with pytest.raises(ValueError, match="table"):
        ops.window_attention(z(1, 4, 4, 12), z(48, 2), 2, 4, 0)
