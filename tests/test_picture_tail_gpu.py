"""The picture tail has three producers of the final 8-bit picture -- the plain tail (k_to_u8 / k_ycc_to_rgb), the stitch
of tiled results (k_tile_stitch) and the merge of the self-ensemble (k_dihedral_merge) -- and one definition of what
they write (csrc/color_common.h).  For one fp32 picture they must write the same bytes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _picture(c, h, w, seed):
    """multiples of 1/256 in [-0.25, 1.25] -- the ordered sum of eight copies and its eighth are then exact in fp32, and
    the clamp works on both sides -- with one NaN"""
    k = np.random.RandomState(seed).randint(-64, 321, size=(1, c, h, w))
    x = torch.from_numpy(k.astype(np.float32) / 256)
    x[0, c - 1, h // 2, w // 3] = float("nan")
    return x


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("kind", ["y", "y_chroma", "rgb"])
@pytest.mark.parametrize("hw", [(33, 47), (17, 250)])   # one pixel over the 32-pixel dihedral tile, widths off the
def test_the_three_producers_write_the_same_bytes(gpu, hw, kind, layout):   # 16-pixel run, tile rows shorter than a run
    from pytorch_super_resolution_model_collection_amd import ops, tiling
    h, w = hw
    c = 3 if kind == "rgb" else 1
    x = _picture(c, h, w, 7 * h + c).to(gpu)
    assert bool(torch.isnan(x).any()) and float(x.nan_to_num(0.5).min()) < 0 and float(x.nan_to_num(0.5).max()) > 1
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    cb = cr = None
    if kind == "y_chroma":
        cb, cr = torch.from_numpy(np.random.RandomState(h).randint(0, 256, size=(2, h, w), dtype=np.uint8)).to(gpu)

    plain = ops.to_u8_image(x) if cb is None else ops.ycbcr_to_rgb_u8(x, cb, cr)
    assert tuple(plain.shape) == (h, w, 3 if cb is not None else c) and int(plain.min()) == 0 and int(plain.max()) == 255

    # tiles of 20 pixels with no overlap and no scaling (2 x 3 and 1 x 13 of them), stitched in two chunks
    plan = tiling.plan(tiling.Geometry(1, 0, 0, 0), h, w, 20)
    assert plan.ntiles > 1 and (plan.OH, plan.OW) == (h, w)
    tp = ops.TilePlan(plan, gpu)
    half = plan.ntiles // 2
    tiled = None
    for t0, n in ((0, half), (half, plan.ntiles - half)):
        tiled = ops.tile_stitch_u8(ops.tile_gather(x, tp, t0, n), tp, t0, tiled, cb, cr)
    assert torch.equal(tiled, plain)

    # the mean of the eight variants of the picture, each turned back: the picture
    merged = ops.dihedral_merge_u8(*ops.dihedral_variants(x), cb=cb, cr=cr)
    assert torch.equal(merged, plain)
