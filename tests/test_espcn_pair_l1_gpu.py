"""k_espcn_pair's tile walk (csrc/conv_pair.hip) carries the tile coordinates (image, tile column, tile
row) along the run by add and carry instead of dividing the tile number in every tile, and its first layer requests its
cells a K step ahead of their MFMAs; nothing that is summed, or in which order, changes: the output is the parent
commit's, bit for bit.

The goldens under tests/golden/espcn_pair_l1/ were written with the library of the parent commit b6e87cc ("Fused losses:
one seed contract for the five loss Functions"), built from that commit's csrc/, by
    SRK_LIB_PATH=/path/to/b6e87cc/libsrk.so python tools/pair_l1_golden.py
Outputs under 1 MB are kept whole; of larger ones a fixed seeded choice of output rows per image, and the SHA-256 of the
whole output's bytes beside them.  The shapes are the smallest that reach each branch the coordinate walk can break."""
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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "espcn_pair_l1")
# N x 3 x H x W -> (seed of the input, factor on it = the declared maximum, output rows kept per image where not whole)
CASES = {
    # OH 17: three tile rows, the last with vr = 1 (both dead-row branches); OW 33: a one-column last tile; every block
    # one tile, so all are fresh
    (1, 3, 23, 39): (31, 1.0, 0),
    # 384 tiles on 256 blocks: runs of one and two tiles, and handed kept rows
    (3, 3, 134, 134): (32, 1.0, 8),
    # tiles_y = 2, so column tops every other tile; image boundaries fall inside runs.  Exponents not those of [0, 1]
    (5, 3, 15, 150): (33, 37.5, 0),
    # tiles_x = 1, tiles_y = 33: long columns, a run crossing an image boundary at a column top
    (2, 3, 270, 22): (34, 1.0, 64),
}
WHOLE_BYTES = 1000 * 1000    # outputs under this size are stored whole


def name_of(shape):
    return "x".join(map(str, shape))


@functools.lru_cache(maxsize=None)
def net():
    ora = fill.fill_module(R.ESPCN(3, 64, 4))
    n = models.ESPCNNet(3, 64, 4)
    n.load_state_dict(ora.state_dict())
    return n.cuda().eval()


def input_of(shape):
    seed, factor, _ = CASES[shape]
    x = (fill.rand(shape, seed) * factor).cuda()
    return ops.declare_absmax(x, factor)


def rows_of(shape):
    """The kept output rows: [N][k] indices, sorted per image, from the case's seed."""
    seed, _, k = CASES[shape]
    rs = np.random.RandomState(1000 + seed)
    return np.stack([np.sort(rs.choice(shape[2] - 6, size=k, replace=False)) for _ in range(shape[0])])


def pick_rows(y, rows):
    """[N][32][k][OW] of an NCHW-shaped output."""
    return torch.stack([y[n][:, torch.from_numpy(rows[n]).to(y.device)] for n in range(y.shape[0])]).contiguous()


def nhwc_bytes(y):
    return np.ascontiguousarray(y.permute(0, 2, 3, 1).cpu().numpy()).tobytes()


def run_pair(x):
    """One forced launch with the declared maximum; no ring timeout, no block on the scan path."""
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


@pytest.mark.parametrize("shape", list(CASES), ids=name_of)
def test_bit_identical_to_parent(shape):
    y = run_pair(input_of(shape))
    n, _, h, w = shape
    assert tuple(y.shape) == (n, 32, h - 6, w - 6)
    if y.numel() * 4 < WHOLE_BYTES:
        want = torch.from_numpy(np.load(os.path.join(GOLDEN, name_of(shape) + ".npy")))
        assert torch.equal(y.cpu(), want), "max |diff| %g" % (y.cpu() - want).abs().max().item()
    else:
        rows = rows_of(shape)
        want = torch.from_numpy(np.load(os.path.join(GOLDEN, name_of(shape) + "_rows.npy")))
        got = pick_rows(y, rows).cpu()
        assert want.numel() * 4 < WHOLE_BYTES
        assert torch.equal(got, want), "kept rows: max |diff| %g" % (got - want).abs().max().item()
        with open(os.path.join(GOLDEN, name_of(shape) + ".json")) as f:
            assert hashlib.sha256(nhwc_bytes(y)).hexdigest() == json.load(f)["sha256"]
