"""k_espcn_pair's software pipeline (csrc/conv_pair.hip) changes when fragments are requested, never what is
summed or in which order: its output is the parent commit's, bit for bit.  The goldens under
tests/golden/espcn_pair_pipeline/ were written by tools/pair_pipeline_golden.py with the parent commit's library; small
outputs are kept whole, large ones as the SHA-256 of their bytes and a 4 KB corner."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import fill, ref_modules as R
from pytorch_super_resolution_model_collection_amd import _lib, models, ops

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "espcn_pair_pipeline")
# N x 3 x H x W -> seed of the input
CASES = {
    (3, 3, 7, 7): 21,        # one tile per image, every tile fresh, no hand-over
    (1, 3, 23, 39): 22,      # OH = 17: three tile rows, the last with vr = 1 (both dead-row branches); three columns
    (2, 3, 38, 22): 23,      # OH = 32: no dead rows, two columns, runs of one tile
    (4, 3, 104, 262): 24,    # 832 tiles on 256 blocks: runs of 3 - 4 tiles, column tops inside runs, last row vr = 2
    (4, 3, 110, 262): 25,    # the same with a full last row (vr = 8)
}
WHOLE_BYTES = 256 * 1024     # outputs up to this size are stored whole
FP64_SHAPE = (1, 3, 23, 39)
REPLAY_SHAPE = (4, 3, 104, 262)


def name_of(shape):
    return "x".join(map(str, shape))


@functools.lru_cache(maxsize=None)
def net():
    ora = fill.fill_module(R.ESPCN(3, 64, 4))
    n = models.ESPCNNet(3, 64, 4)
    n.load_state_dict(ora.state_dict())
    return n.cuda().eval()


def input_of(shape):
    return fill.rand(shape, CASES[shape]).cuda()


def run_pair(x):
    """One forced launch; no ring timeout, no block on the scan path."""
    lib = _lib.load()
    assert lib.srk_ring_timeouts(1) >= 0 and lib.srk_espcn_pair_scans(1) >= 0
    with torch.no_grad():
        y = ops.espcn_pair(x, net().layers[0], net().layers[1], force=True)
    assert y is not None
    assert lib.srk_last_kernel_name().decode() == "k_espcn_pair"
    torch.cuda.synchronize()
    assert lib.srk_ring_timeouts(1) == 0
    assert lib.srk_espcn_pair_scans(1) == 0
    return y


def nhwc_bytes(y):
    return np.ascontiguousarray(y.permute(0, 2, 3, 1).cpu().numpy()).tobytes()


def corner(y):
    """The last image's bottom right 4 x 8 pixels, 32 channels: 4 KB."""
    return y[-1, :, -4:, -8:].contiguous().cpu().numpy()


@pytest.mark.parametrize("shape", list(CASES), ids=name_of)
def test_bit_identical_to_parent(shape):
    y = run_pair(input_of(shape))
    n, _, h, w = shape
    assert tuple(y.shape) == (n, 32, h - 6, w - 6)
    if y.numel() * 4 <= WHOLE_BYTES:
        want = torch.from_numpy(np.load(os.path.join(GOLDEN, name_of(shape) + ".npy")))
        assert torch.equal(y.cpu(), want), "max |diff| %g" % (y.cpu() - want).abs().max().item()
    else:
        with open(os.path.join(GOLDEN, name_of(shape) + ".json")) as f:
            want = json.load(f)
        got_c, want_c = corner(y), np.load(os.path.join(GOLDEN, name_of(shape) + "_corner.npy"))
        assert want_c.nbytes == 4096
        assert np.array_equal(got_c, want_c), "corner: max |diff| %g" % np.abs(got_c - want_c).max()
        assert hashlib.sha256(nhwc_bytes(y)).hexdigest() == want["sha256"]


def test_replay_is_bit_identical_to_eager():
    x = input_of(REPLAY_SHAPE)
    eager = run_pair(x).clone()
    lib = _lib.load()
    static = x.clone()
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.no_grad():
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                y = ops.espcn_pair(static, net().layers[0], net().layers[1], force=True)
        assert y is not None
        for _ in range(3):
            y.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager)
    assert lib.srk_ring_timeouts(1) == 0
    assert lib.srk_espcn_pair_scans(1) == 0


def test_against_fp64():
    """The bar of tests/test_espcn_pair_gpu.py for the same quantity: no more than 1.5 times the two-launch path's error
    against the convolution in double (maximum and rms, relative to max |ref|), and within 1e-5 of that path."""
    x = input_of(FP64_SHAPE)
    y1 = run_pair(x)
    c1, c2 = net().layers[0].conv, net().layers[1].conv
    with torch.no_grad():
        y2 = net().layers[1](net().layers[0](x))
        r = torch.relu(torch.nn.functional.conv2d(x.double(), c1.weight.double(), c1.bias.double()))
        ref = torch.relu(torch.nn.functional.conv2d(r, c2.weight.double(), c2.bias.double()))
    scale = ref.abs().max().item()

    def err(y):
        d = (y.permute(0, 2, 3, 1).double() - ref.permute(0, 2, 3, 1)).abs()
        return d.max().item() / scale, d.pow(2).mean().sqrt().item() / scale

    e1, e2 = err(y1), err(y2)
    print("pair max %.3e rms %.3e   two launches max %.3e rms %.3e" % (e1 + e2))
    assert e1[0] <= 1.5 * e2[0] + 1e-7 and e1[1] <= 1.5 * e2[1] + 1e-8, (e1, e2)
    assert (y1 - y2).abs().max().item() <= 1e-5 * y2.abs().max().item()
