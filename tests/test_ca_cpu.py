"""Channel attention without a GPU: srk_channel_attention_host (the kernels' MLP bodies, csrc/ca_common.h, in plain C++
double) against the fp64 restatement of tests/ca_ref.py over the issue's case table, the planner, and the argument and
range checks of every entry point.  The device kernels are held to the same table in tests/test_ca_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__
import ca_ref as R

# both sides are fp64 on the same fp32 inputs: only summation order and exp() differ
HOST_TOL = 1e-12


@pytest.fixture(scope="module")
def lib():
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as p
    return p._lib.load()


@pytest.mark.parametrize("skip", (False, True))
@pytest.mark.parametrize("name", R.cases())
def test_restatement_matches_autograd(name, skip):
    """The written-out backward is torch autograd's of the plain composition; dL/dx is g."""
    case = R.make(name, skip)
    want = R.autograd(case)
    got = R.restate(case)
    for what, a, b in zip(("y", "dt", "dw1", "db1", "dw2", "db2"), got[:6], (want[0], want[1]) + want[3:]):
        assert R.worst(a, b) <= 1e-13, (name, what, R.worst(a, b))
    if skip:
        assert torch.equal(want[2], case.g.double())


@pytest.mark.parametrize("skip", (False, True))
@pytest.mark.parametrize("name", R.cases())
def test_host_twin_matches_restatement(lib, name, skip):
    case = R.make(name, skip)
    want, got = R.restate(case), R.host(lib, case)
    for what in ("y", "dt", "dw1", "db1", "dw2", "db2"):
        err = R.worst(getattr(got, what), getattr(want, what))
        print("srk_channel_attention_host %-12s skip %d %-4s worst %.3g of max |ref|" % (name, skip, what, err))
        assert err <= HOST_TOL, (name, what, err)
    if name == "dead_hidden":   # h = 0: nothing reaches the first layer, and the second layer's weights see h = 0
        assert float(want.h.abs().max()) == 0.0
        for what in ("dw1", "db1", "dw2"):
            assert float(getattr(got, what).abs().max()) == 0.0, what
        # dm = 0, so dt = g * s with s = sigmoid(b2) (the two sides' exp() may differ in the last bit)
        assert R.worst(got.dt, case.g.double() * want.s[:, :, None, None]) <= 1e-15
    if name == "saturated":
        # sigmoid(40) is 1 in fp64 and fp32, so s (1 - s) = 0 exactly on the +40 half; sigmoid(-40) = 4.2e-18 is a normal
        # number in both formats, so on the -40 half s (1 - s) = s: not an exact zero.  |W2 h| <= 10 there (two hidden
        # units, weights of std 0.5), so s <= sigmoid(-30) < 1e-13, and dm, a few hundred products of it, stays below 1e-9
        c = case.t.shape[1]
        assert bool((want.s[:, :c // 2] == 1.0).all()) and float(want.s[:, c // 2:].max()) < 1e-13
        dm = got.dt - case.g.double() * want.s[:, :, None, None]
        assert float(dm.abs().max()) < 1e-9
        assert torch.equal(got.dt[:, :c // 2].float(), case.g[:, :c // 2])      # to fp32, dt = g * s there
        assert float(got.db2[:c // 2].abs().max()) == 0.0 and float(got.dw2[:c // 2].abs().max()) == 0.0


def test_forward_only(lib):
    case = R.make("scalar", True)
    assert torch.equal(R.host(lib, case, backward=False).y, R.host(lib, case).y)


def test_a_nan_stays_in_its_sample(lib):
    case = R.make("scalar", True)
    clean = R.host(lib, case)
    case.t[1, 2, 3, 4] = float("nan")
    got = R.host(lib, case)
    for what in ("y", "dt"):
        a, b = getattr(got, what), getattr(clean, what)
        assert torch.isnan(a[1]).all(), what                 # the mean, hence every gate, of sample 1
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]), what


def test_planner(lib):
    """One partial a sample for small maps, several for large ones, both present in the table; the workspace holds the
    partials of either direction and what the parameter-gradient launch reads."""
    splits = {name: lib.srk_channel_attention_splits(v[0], v[3], v[4], v[1]) for name, v in R.TABLE.items()}
    assert min(splits.values()) == 1 and max(splits.values()) > 1, splits
    assert splits["hw1"] == 1 and splits["wide"] > 1 and splits["patch"] > 1
    for name, (n, c, cr, h, w) in R.TABLE.items():
        assert lib.srk_channel_attention_workspace(n, h, w, c) >= 8 * (n * splits[name] * c + n * c + n * cr)
    assert lib.srk_channel_attention_splits(1, 2000, 2000, 64) == lib.srk_channel_attention_splits(1, 4000, 4000, 64)  # capped
    assert lib.srk_channel_attention_splits(7, 40, 40, 64) == splits["patch"]     # a sample's own affair


def test_argument_and_range_checks(lib):
    buf = np.zeros(1 << 16, np.float32)
    out = np.zeros(1 << 16, np.float64)
    p, o = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    err = lambda: lib.srk_last_error_string()

    def fwd(t=p, w1=p, y=p, ws=p, n=2, h=4, w=4, c=8, cr=2, nbytes=1 << 16):
        return lib.srk_channel_attention_forward(t, None, w1, p, p, p, n, h, w, c, cr, y, None, None, None, ws, nbytes, None)

    def bwd(g=p, dt=p, ws=p, n=2, h=4, w=4, c=8, cr=2, nbytes=1 << 16):
        return lib.srk_channel_attention_backward(g, p, p, p, p, p, p, n, h, w, c, cr, dt, None, None, None, None, 0.0, ws,
                                                  nbytes, None)

    def host(t=p, y=o, n=2, h=4, w=4, c=8, cr=2, g=None, dt=None):
        return lib.srk_channel_attention_host(t, None, p, p, p, p, g, n, h, w, c, cr, y, dt, None, None, None, None)

    # (all refused before anything is launched or read: no device is needed for these)
    for call in (fwd, bwd, host):
        assert call(n=0) == -1 and b"bad dims" in err()
        assert call(h=-1) == -1 and call(w=0) == -1 and call(c=0) == -1 and call(cr=0) == -1
        assert call(c=8, cr=9) == -1 and b"Cr = 9 exceeds C = 8" in err()
        assert call(c=257, cr=4) == -2 and b"SRK_CA_MAX_C = 256" in err()
        assert call(c=256, cr=65) == -2 and b"SRK_CA_MAX_CR = 64" in err()
        assert lib.srk_status_string(-2) == lib.srk_status_string(call(c=512, cr=8))
    assert fwd(t=None) == -1 and b"null pointer" in err()
    assert fwd(w1=None) == -1 and fwd(y=None) == -1 and fwd(ws=None) == -1
    assert bwd(g=None) == -1 and bwd(dt=None) == -1 and bwd(ws=None) == -1 and b"null pointer" in err()
    assert host(t=None) == -1 and host(y=None) == -1
    assert host(g=p) == -1 and b"a backward needs" in err()
    assert fwd(nbytes=8) == -4 and b"workspace" in err() and bwd(nbytes=8) == -4
    assert lib.srk_channel_attention_forward(p, None, p, p, p, p, 2, 4, 4, 8, 2, p, p, None, None, p, 1 << 16, None) == -1
    assert b"saved together" in err()
    assert lib.srk_channel_attention_splits(0, 4, 4, 8) == -1 and lib.srk_channel_attention_splits(1, 4, 4, 300) == -2
    assert lib.srk_channel_attention_workspace(1, 0, 4, 8) == 0 and lib.srk_channel_attention_workspace(1, 4, 4, 300) == 0
    assert lib.srk_version() == 600
