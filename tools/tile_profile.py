#!/usr/bin/env python3
"""Evidence for DESIGN 17 (tiled super-resolution of pictures), run on the MI355X box from the repo root:

  python tools/tile_profile.py prepare DIR        the seeded 510 x 339 picture and the VDSR (Y) / EDSR (RGB) checkpoints of
                                                  tools/test_single_profile.py under DIR
  python tools/tile_profile.py sweep MODEL DIR    one pass against tile in {128, 192, 256, 384} x tile_batch in {4, 16, all}
                                                  on that picture: net time (HIP events around upload-free _forward: gather,
                                                  net, stitch) and whole test_single(path) time (host clock: decode, upload,
                                                  device work, the one copy back, PNG encode)
  python tools/tile_profile.py stitch             k_tile_stitch writing 8 bits against tile_stitch + k_to_u8 / k_ycc_to_rgb
                                                  on the 2040 x 1356 output
  python tools/tile_profile.py big tiled|onepass  EDSR x4 on a synthetic 1020 x 678 picture, whose x4 feature map is past
                                                  2^31 bytes: time and peak memory (or the error text; a failure is not
                                                  retried); run each side in a process of its own

Medians over warm runs on one box; one pass with tile=None is the code of the parent commit, unchanged."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, SCALE = 510, 339, 4
TILES, BATCHES, REPS = (128, 192, 256, 384), (4, 16, "all"), 7


def _trainer(model, d):
    import __graft_entry__
    __graft_entry__.build()
    from tools.test_single_profile import _args
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    t = TRAINERS[model](_args(model, d))
    t.model = t.build_model().to(t.device)
    t.load_model()
    return t


def _events(fn, reps=REPS, warm=2):
    """median / min of `reps` device-event timings of fn() in ms, after `warm` untimed calls"""
    import torch
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def _wall(fn, reps=5, warm=1):
    for _ in range(warm):
        fn()
    s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        s.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(s), min(s)


def sweep(model, d):
    import numpy as np
    import torch
    from PIL import Image
    from pytorch_super_resolution_model_collection_amd import tiling
    t = _trainer(model, d)
    fn = os.path.join(d, "picture.png")
    rgb = np.asarray(Image.open(fn).convert("RGB"))
    if model == "VDSR":
        x = torch.from_numpy(np.asarray(Image.open(fn).convert("YCbCr"))[:, :, 0].copy()).float().div(255).view(1, 1, H, W)
    else:
        x = torch.from_numpy(rgb.copy()).float().div(255).permute(2, 0, 1).contiguous().view(1, 3, H, W)
    x = x.to(t.device)
    geo = tiling.net_geometry(t.model.eval())
    xin = t._net_input(x)
    print("== %s x%d, picture %d x %d, net input %d x %d, reach %s input pixels, widest activation %.2f GB in one pass"
          % (model, SCALE, W, H, xin.shape[-1], xin.shape[-2], geo.reach,
             tiling.activation_bytes(geo, xin.shape[-2], xin.shape[-1]) / 2 ** 30))
    print("%-6s %-6s %-7s %-22s %-22s %-10s" % ("tile", "batch", "tiles", "net ms (median, min)", "whole ms (median, min)", "peak GB"))
    ref = t._forward(x)

    def row(tile, tb):
        torch.cuda.reset_peak_memory_stats()
        net = _events(lambda: t._forward(x, tile, tb))
        peak = torch.cuda.max_memory_allocated() / 2 ** 30
        whole = _wall(lambda: t.test_single(fn, tile=tile, tile_batch=tb))
        n = 1 if tile is None else tiling.plan(geo, xin.shape[-2], xin.shape[-1], tile).ntiles
        if tile is not None:
            err = float((t._forward(x, tile, tb) - ref).abs().max())
            assert err < 1e-4, err
        print("%-6s %-6s %-7d %8.3f %8.3f      %8.2f %8.2f      %8.2f" % (tile or "-", tb if tile else "-", n, net[0], net[1],
                                                                         whole[0], whole[1], peak))
    row(None, None)
    for tile in TILES:
        for tb in BATCHES:
            row(tile, tb)
    row(None, None)   # one pass again: the spread of the box over the sweep


def stitch():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd import ops, tiling
    dev = torch.device("cuda", 0)
    plan = tiling.plan(tiling.Geometry(4, 0, -143, 143), H, W, 192)      # EDSR x4 tiles of the 510 x 339 picture
    tp = ops.TilePlan(plan, dev)
    px = plan.OH * plan.OW
    print("== stitch to 8 bits, %d x %d output from %d tiles of %d x %d; bytes are what the algorithm needs; share of 8 TB/s"
          % (plan.OW, plan.OH, plan.ntiles, plan.otw, plan.oth))
    g = torch.Generator().manual_seed(3)
    cbcr = torch.randint(0, 256, (2, plan.OH, plan.OW), dtype=torch.uint8, generator=g).to(dev)
    for c, chroma in ((1, True), (3, False)):
        tiles = torch.rand((plan.ntiles, c, plan.oth, plan.otw), generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        cb, cr = (cbcr[0], cbcr[1]) if chroma else (None, None)
        out8 = torch.empty((plan.OH, plan.OW, 3), dtype=torch.uint8, device=dev)
        pic = torch.empty((c, plan.OH, plan.OW), dtype=torch.float32, device=dev)
        fused = lambda: ops.tile_stitch_u8(tiles, tp, 0, out8, cb, cr)
        if chroma:
            two = lambda: ops.ycbcr_to_rgb_u8(ops.tile_stitch(tiles, tp, 0, pic), cb, cr)
        else:
            two = lambda: ops.to_u8_image(ops.tile_stitch(tiles, tp, 0, pic))
        assert torch.equal(fused(), two())
        n_in = 4 * c + (2 if chroma else 0)
        bytes_f, bytes_t = px * (n_in + 3), px * (4 * c + 4 * c) + px * (n_in + 3)
        res = {"fused": [], "two launches": []}
        for _ in range(5):                                     # alternate the two forms
            for name, fn in (("fused", fused), ("two launches", two)):
                res[name].append(_events(lambda: [fn() for _ in range(20)], reps=3, warm=1)[0] / 20)
        for name, b in (("fused", bytes_f), ("two launches", bytes_t)):
            m = statistics.median(res[name])
            print("C = %d%s  %-13s median %7.2f us (min %7.2f) per call incl. launch; %6.1f MB; %5.1f %% of 8 TB/s"
                  % (c, " + chroma" if chroma else "         ", name, m * 1e3, min(res[name]) * 1e3, b / 1e6, b / (m * 1e-3) / 8e12 * 100))


def big(side):
    import torch
    from pytorch_super_resolution_model_collection_amd import tiling
    import tempfile
    d = tempfile.mkdtemp()
    from tools.test_single_profile import _args
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    torch.manual_seed(1)
    t = TRAINERS["EDSR"](_args("EDSR", d))
    t.model = t.build_model()
    t.model.weight_init()
    t.model.to(t.device).eval()
    g = torch.Generator().manual_seed(7)
    x = torch.rand((1, 3, 678, 1020), generator=g).to(t.device)
    geo = tiling.net_geometry(t.model)
    print("== EDSR x4, synthetic 1020 x 678 picture, %s; widest activation in one pass %.2f GB (limit of the fast kernels: 2 GB)"
          % (side, tiling.activation_bytes(geo, 678, 1020) / 2 ** 30), flush=True)
    tile = None if side == "onepass" else tiling.resolve_tile("auto", geo, 678, 1020)
    t._forward(x[:, :, :96, :96].contiguous(), None)       # warm: code objects, filter packing
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(4):   # the first run of this shape, then three warm ones
        t0 = time.perf_counter()
        try:
            out = t._forward(x, tile)
            torch.cuda.synchronize()
        except Exception as e:   # recorded, not retried
            print("%s: %s: %s" % (side, type(e).__name__, str(e)[:500]))
            return
        ms.append((time.perf_counter() - t0) * 1e3)
    print("%s (tile %s, batch %s): first run %.1f ms, then median %.1f ms (host clock around a synchronise), peak memory %.2f GB, "
          "output %s, finite %s, mean %.6f"
          % (side, tile, tiling.DEFAULT_TILE_BATCH if tile else "-", ms[0], statistics.median(ms[1:]),
             torch.cuda.max_memory_allocated() / 2 ** 30, tuple(out.shape), bool(torch.isfinite(out).all()), float(out.double().mean())))


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "prepare":
        from tools.test_single_profile import prepare
        prepare(sys.argv[2])
    elif mode == "sweep":
        sweep(sys.argv[2], sys.argv[3])
    elif mode == "stitch":
        stitch()
    elif mode == "big":
        big(sys.argv[2])
