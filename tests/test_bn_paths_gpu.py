"""Every launch plan of the BatchNorm family (csrc/bn_linear.hip, ops._BatchNorm / _InstanceNorm) gives the parent commit's
results, bit for bit: the kernels share one copy of each reduction, finalize and dx formula, which may change
where an operation is written but never which operations run or in which order.  The goldens under tests/golden/bn_paths/
were written by tools/bn_paths_golden.py with the parent commit's tree and library; tensors up to 64 KB are kept whole,
larger ones as the SHA-256 of their bytes and a corner.

The second half checks through the C ABI what the shared backward column-sum launcher repaired: the _act entry points with
SRK_ACT_NONE are the plain BatchNorm backward, not a LeakyReLU one."""
import contextlib
import hashlib
import json
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import fill
from pytorch_super_resolution_model_collection_amd import _lib, ops

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_paths")
WHOLE_BYTES = 64 * 1024
KEYS = ("y", "mean", "rstd", "running_mean", "running_var", "dx", "dgamma", "dbeta", "dprelu")


def _case(kind, shape, act="none", fin=True, red16=True, calls=1):
    return {"kind": kind, "shape": shape, "act": act, "fin": fin, "red16": red16, "calls": calls}


# the smallest shapes at which each launch plan is chosen.  A single PReLU slope (prelu1) on the separate launches is one
# float atomic per 64-channel block: exact from run to run only for C <= 64 -- every prelu1 case here has C <= 64.
CASES = (
    # scalar kernels (C % 4 != 0)
    [_case(k, (2, 6, 5, 7)) for k in ("train", "eval")]
    # float4 kernels, no fused finalize (C % 16 != 0)
    + [_case("train", (3, 8, 7, 9), a) for a in ("none", "lrelu", "prelu1", "preluC", "none+res", "prelu1+res")]
    + [_case("eval", (3, 8, 7, 9), a) for a in ("none", "lrelu")]
    # the same with more than 64 row splits, in the three-sum backward too (rows > 8192)
    + [_case("train", (2, 12, 66, 63), a) for a in ("none", "lrelu", "preluC", "prelu1")]
    # finalize-in-apply: one slab; three slabs with a ragged last row range
    + [_case("train", s, a) for s in ((5, 16, 9, 11), (3, 48, 37, 20)) for a in ("none", "lrelu", "prelu1", "preluC+res")]
    # a shape the fused finalize takes, on the separate launches (narrow k_bn_reduce_fused<., 4>)
    + [_case("train", (5, 16, 9, 11), a, fin=False) for a in ("none", "lrelu")]
    # the 64-channel reduce blocks (SRK_BN_RED16 = 0)
    + [_case("train", (2, 12, 66, 63), red16=False)]
    # BatchNorm1d [B, F]
    + [_case("train", (24, 10)), _case("train", (24, 10), calls=2), _case("eval", (24, 10))]
    # InstanceNorm
    + [_case("instance", s) for s in ((2, 6, 5, 7), (2, 8, 6, 6))]
)


def name_of(case):
    n = "%s_%s_%s" % (case["kind"], "x".join(map(str, case["shape"])), case["act"].replace("+", "_"))
    return n + ("" if case["fin"] else "_sep") + ("" if case["red16"] else "_red64") + ("_x%d" % case["calls"] if case["calls"] > 1 else "")


def _seed(case):
    return 1000 + zlib.crc32(name_of(case).encode()) % 100000   # (of the name: adding a case moves no other case's inputs)


def _dev(t, shape):
    t = t.cuda()
    return t.contiguous(memory_format=torch.channels_last) if len(shape) == 4 else t


@contextlib.contextmanager
def _switches(fin, red16):
    prev_fin, prev_env = ops.BN_FIN_APPLY, os.environ.get("SRK_BN_RED16")
    ops.BN_FIN_APPLY = fin
    os.environ["SRK_BN_RED16"] = "1" if red16 else "0"
    try:
        yield
    finally:
        ops.BN_FIN_APPLY = prev_fin
        if prev_env is None:
            del os.environ["SRK_BN_RED16"]
        else:
            os.environ["SRK_BN_RED16"] = prev_env


def run_case(case):
    """The case's forward and backward through ops.batch_norm / ops.instance_norm: {key of KEYS: tensor}."""
    shape, seed = case["shape"], _seed(case)
    c = shape[1]
    x = _dev(fill.randn(shape, seed) * 1.7 + 0.3, shape).requires_grad_(True)
    dy = _dev(fill.randn(shape, seed + 1), shape)
    if case["kind"] == "instance":
        y = ops.instance_norm(x)
        _, mean, rstd = y.grad_fn.saved_tensors
        y.backward(dy)
        return {"y": y.detach(), "mean": mean, "rstd": rstd, "dx": x.grad}
    kind = case["act"].split("+")[0]
    code = {"none": _lib.ACT_NONE, "lrelu": _lib.ACT_LRELU, "prelu1": _lib.ACT_PRELU, "preluC": _lib.ACT_PRELU}[kind]
    gamma = fill.rand((c,), seed + 2, 0.5, 1.5).cuda().requires_grad_(True)
    beta = (fill.randn((c,), seed + 3) * 0.3).cuda().requires_grad_(True)
    pw = fill.rand((1 if kind == "prelu1" else c,), seed + 4, 0.1, 0.4).cuda().requires_grad_(True) if code == _lib.ACT_PRELU else None
    res = _dev(fill.randn(shape, seed + 5), shape) if case["act"].endswith("+res") else None
    rm = fill.randn((c,), seed + 6).cuda() * 0.2
    rv = fill.rand((c,), seed + 7, 0.5, 1.5).cuda()
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    training = case["kind"] == "train"
    assert code == _lib.ACT_NONE or ops.bn_fusable(x, code, pw)
    with _switches(case["fin"], case["red16"]):
        for _ in range(case["calls"]):   # (BatchNorm applied twice: the running statistics move twice)
            y = ops.batch_norm(x, gamma, beta, rm, rv, training, 0.1, 1e-5, None, nbt, code, 0.2, pw, res)
        _, _, mean, rstd, _, _ = y.grad_fn.saved_tensors
        y.backward(dy)
    assert int(nbt) == (case["calls"] if training else 0)
    out = {"y": y.detach(), "mean": mean, "rstd": rstd, "running_mean": rm, "running_var": rv, "dx": x.grad,
           "dgamma": gamma.grad, "dbeta": beta.grad}
    if pw is not None:
        out["dprelu"] = pw.grad
    return out


def to_numpy(t):
    """Host copy in memory order: [N][H][W][C] for a 4-D tensor (the kernels' layout)."""
    t = t.detach()
    return np.ascontiguousarray((t.permute(0, 2, 3, 1) if t.dim() == 4 else t).cpu().numpy())


def corner(a):
    """The last image's bottom right 4 x 8 pixels, every channel (of to_numpy's [N][H][W][C])."""
    return np.ascontiguousarray(a[-1, -4:, -8:, :])


def digest(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


@pytest.mark.parametrize("case", CASES, ids=name_of)
def test_bit_identical_to_parent(gpu, case):
    got = {k: to_numpy(v) for k, v in run_case(case).items()}
    assert set(got) <= set(KEYS)
    want = np.load(os.path.join(GOLDEN, name_of(case) + ".npz"), allow_pickle=False)
    with open(os.path.join(GOLDEN, "sha256.json")) as f:
        hashes = json.load(f).get(name_of(case), {})
    assert set(got) == {k[:-len("_corner")] if k.endswith("_corner") else k for k in want.files}
    for k, a in got.items():
        if a.nbytes <= WHOLE_BYTES:
            assert a.shape == want[k].shape
            assert torch.equal(torch.from_numpy(a), torch.from_numpy(want[k])), "%s: max |diff| %g" % (k, np.abs(a - want[k]).max())
        else:
            assert torch.equal(torch.from_numpy(corner(a)), torch.from_numpy(want[k + "_corner"])), k + " corner"
            assert digest(a) == hashes[k], k


# ---- the _act backward entry points with SRK_ACT_NONE ---------------------------------------------------------------------
def _backward_inputs(shape, seed, offset=0):
    """dy, x ([rows][C], optionally views at a 4-byte offset), mean, rstd, gamma, beta on the device."""
    n, c, h, w = shape
    rows = n * h * w

    def rows_c(s):
        base = torch.zeros(rows * c + 4, device="cuda")
        v = base[offset:offset + rows * c].view(rows, c)
        v.copy_(fill.randn((rows, c), s).cuda())
        return v

    dy, x = rows_c(seed), rows_c(seed + 1)
    mean = (fill.randn((c,), seed + 2) * 0.3).cuda()
    rstd = fill.rand((c,), seed + 3, 0.5, 1.5).cuda()
    gamma = fill.rand((c,), seed + 4, 0.5, 1.5).cuda()
    beta = (fill.randn((c,), seed + 5) * 0.3).cuda()
    return rows, c, dy, x, mean, rstd, gamma, beta


@pytest.mark.parametrize("shape", [(3, 8, 7, 9), (2, 12, 66, 63)], ids=lambda s: "x".join(map(str, s)))
def test_stats_grads_act_without_activation_is_the_plain_backward(gpu, shape):
    """srk_bn_backward_stats_grads_act(SRK_ACT_NONE, slope = 0.2) must not mask dy by the sign of z: its sums and parameter
    gradients are those of srk_bn_backward_stats_grads, bit for bit."""
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream_ptr
    rows, c, dy, x, mean, rstd, gamma, beta = _backward_inputs(shape, 700 + shape[1])
    ws = torch.empty(int(lib.srk_bn_workspace_bytes(c)), dtype=torch.uint8, device="cuda")
    out = []
    for through_act in (False, True):
        dstats = torch.full((2 * c,), float("nan"), dtype=torch.float64, device="cuda")
        dgamma, dbeta = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
        if through_act:
            rc = lib.srk_bn_backward_stats_grads_act(P(dy), P(x), P(mean), P(rstd), P(gamma), P(beta), P(dstats), rows, c,
                                                     P(dgamma), P(dbeta), _lib.ACT_NONE, 0.2, None, 0, None, P(ws), S())
        else:
            rc = lib.srk_bn_backward_stats_grads(P(dy), P(x), P(mean), P(rstd), P(dstats), rows, c, P(dgamma), P(dbeta),
                                                 P(ws), S())
        assert rc == 0
        torch.cuda.synchronize()
        out.append((dstats, dgamma, dbeta))
    for a, b, what in zip(out[0], out[1], ("dstats", "dgamma", "dbeta")):
        assert torch.equal(a, b), "%s: max |diff| %g" % (what, (a - b).abs().max().item())


def test_backward_apply_act_without_activation_on_an_unaligned_view(gpu):
    """srk_bn_backward_apply_act(SRK_ACT_NONE) on tensors at a 4-byte offset takes the scalar kernel and equals
    srk_bn_backward_apply; with an activation such tensors are still refused."""
    lib, P, S = _lib.load(), _lib.ptr, _lib.stream_ptr
    rows, c, dy, x, mean, rstd, gamma, beta = _backward_inputs((3, 8, 7, 9), 720, offset=1)
    assert dy.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 4
    dstats = (fill.randn((2 * c,), 726) * 3.0).double().cuda()
    count = float(rows)

    def dx_view():
        return torch.full((rows * c + 4,), float("nan"), device="cuda")[1:1 + rows * c].view(rows, c)

    plain, through_act, refused = dx_view(), dx_view(), dx_view()
    assert lib.srk_bn_backward_apply(P(dy), P(x), P(mean), P(rstd), P(gamma), P(dstats), count, P(plain), rows, c, S()) == 0
    assert lib.srk_bn_backward_apply_act(P(dy), P(x), P(mean), P(rstd), P(gamma), P(beta), P(dstats), count, P(through_act),
                                         rows, c, _lib.ACT_NONE, 0.2, None, 0, S()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(plain).all()
    assert torch.equal(plain, through_act)
    assert lib.srk_bn_backward_apply_act(P(dy), P(x), P(mean), P(rstd), P(gamma), P(beta), P(dstats), count, P(refused),
                                         rows, c, _lib.ACT_LRELU, 0.2, None, 0, S()) != 0
