#!/usr/bin/env python3
"""Evidence for DESIGN 19 (x8 geometric self-ensemble), run on the MI355X box from the repo root:

  python tools/time_ensemble.py kernels [small|large]   k_dihedral_variants and k_dihedral_merge alone, for the net input of
                                              a 510 x 339 (small) and a 2040 x 1356 (large) picture and the x4 output of
                                              each, C = 3 and C = 1: time per call, GB/s of the bytes the algorithm moves,
                                              next to a plain device copy of the same bytes and to the torch composition
                                              each replaces (rot90 / flip / contiguous / cat; stack / mean / to_u8_image
                                              or ycbcr_to_rgb_u8)
  python tools/time_ensemble.py whole MODEL [small|large]   EDSR or ESPCN x4 (seeded weights): the ensemble call against
                                              eight times the single forward of the same picture, one pass and tiled
                                              (tile 384): the tensor form (HIP events around upload-free _forward) and the
                                              device part of the path form (the picture's bytes on the device -> the 8-bit
                                              result on the device: colour split, net, chroma resize, 8-bit tail)

Medians over warm runs on one box, the sides of a comparison alternated."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = {"small": (339, 510), "large": (1356, 2040)}   # (H, W) of the pictures of profiles/test_single_*.txt and tile_*.txt
SCALE, TILE = 4, 384


def _events(fn, reps=5, warm=2):
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


def _compare(sides, inner):
    """{name: fn} -> {name: median ms per call}, five rounds alternating the sides, `inner` calls per timing"""
    res = {k: [] for k in sides}
    for _ in range(5):
        for name, fn in sides.items():
            res[name].append(_events(lambda: [fn() for _ in range(inner)], reps=3, warm=1)[0] / inner)
    return {k: statistics.median(v) for k, v in res.items()}


def kernels(which):
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import ensemble_ref as E
    from pytorch_super_resolution_model_collection_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(3)
    for size in which:
        h, w = SIZES[size]
        inner = 20 if size == "small" else 3
        for c in (3, 1):
            # -- variants of the net input
            x = torch.rand((1, c, h, w), generator=g).to(dev)
            nbytes = 4 * c * h * w * 9                                   # read once, written eight times
            src, dst = torch.empty(nbytes // 8, device=dev), torch.empty(nbytes // 8, device=dev)
            cl = torch.channels_last

            def composed():
                ev = torch.cat([E.transform(x, k).contiguous(memory_format=cl) for k in (0, 2, 4, 6)])
                od = torch.cat([E.transform(x, k).contiguous(memory_format=cl) for k in (1, 3, 5, 7)])
                return ev, od
            var = ops.dihedral_variants(x)
            assert all(torch.equal(a, b) for a, b in zip(var, composed()))
            r = _compare({"k_dihedral_variants": lambda: ops.dihedral_variants(x), "torch composition": composed,
                          "device copy": lambda: dst.copy_(src)}, inner)
            _report("variants C=%d %dx%d" % (c, w, h), nbytes, r, "k_dihedral_variants")
            # -- merge of the x4 outputs
            oh, ow = SCALE * h, SCALE * w
            even = torch.rand((4, c, oh, ow), generator=g).to(dev).contiguous(memory_format=cl)
            odd = torch.rand((4, c, ow, oh), generator=g).to(dev).contiguous(memory_format=cl)
            outs = [(odd if k % 2 else even)[k // 2:k // 2 + 1] for k in range(8)]
            out = torch.empty((1, c, oh, ow), device=dev)

            def composed_f32():
                return torch.stack([E.inverse(y, k) for k, y in enumerate(outs)]).mean(0)
            want = E.mean_in_order([E.inverse(y, k) for k, y in enumerate(outs)])
            assert torch.equal(ops.dihedral_merge(even, odd, out), want)
            assert torch.equal(ops.dihedral_merge_u8(even, odd), ops.to_u8_image(want))
            px = oh * ow
            sides = [("merge f32", px * c * 4 * 9, lambda: ops.dihedral_merge(even, odd, out), composed_f32),
                     ("merge u8 ", px * c * (4 * 8 + 1), lambda: ops.dihedral_merge_u8(even, odd),
                      lambda: ops.to_u8_image(composed_f32()))]
            if c == 1:
                cbcr = torch.randint(0, 256, (2, oh, ow), dtype=torch.uint8, generator=g).to(dev)
                assert torch.equal(ops.dihedral_merge_u8(even, odd, cbcr[0], cbcr[1]), ops.ycbcr_to_rgb_u8(want, cbcr[0], cbcr[1]))
                sides.append(("merge ycc", px * (4 * 8 + 2 + 3), lambda: ops.dihedral_merge_u8(even, odd, cbcr[0], cbcr[1]),
                              lambda: ops.ycbcr_to_rgb_u8(composed_f32(), cbcr[0], cbcr[1])))
            for name, nb, fused, comp in sides:
                src, dst = torch.empty(nb // 8, device=dev), torch.empty(nb // 8, device=dev)
                r = _compare({"k_dihedral_merge": fused, "torch composition": comp, "device copy": lambda: dst.copy_(src)}, inner)
                _report("%s C=%d %dx%d" % (name, c, ow, oh), nb, r, "k_dihedral_merge")
            del even, odd, outs, out, want, src, dst
            torch.cuda.empty_cache()


def _report(what, nbytes, r, fused):
    f = r[fused]
    print("%-28s %8.1f MB moved | %s %8.3f ms %7.0f GB/s | device copy of the same bytes %8.3f ms %7.0f GB/s | torch composition "
          "%8.3f ms = %.2f x the kernel" % (what, nbytes / 1e6, fused, f, nbytes / f / 1e6, r["device copy"],
                                            nbytes / r["device copy"] / 1e6, r["torch composition"], r["torch composition"] / f),
          flush=True)


def _path_device(t, rgb, tile, ens):
    """the device part of _Trainer._test_single_file: uint8 [H,W,3] on the device -> the 8-bit result on the device"""
    from pytorch_super_resolution_model_collection_amd import ops
    h, w = int(rgb.shape[0]), int(rgb.shape[1])
    cbcr = None
    if t.num_channels == 1:
        y, cbcr = ops.rgb_to_ycc_planes(rgb, y_float=True)
        x = y.view(1, 1, h, w)
    else:
        x = ops.resize_u8(rgb.permute(2, 0, 1), h, w, out_float=True).unsqueeze(0)
    x = t._net_input(x)
    size, geo = t._resolve_tile(tile, x, ens)
    if size is not None:
        return t._infer_tiled(x, geo, size, None, as_u8=True, chroma=cbcr, ensemble=ens)
    if ens:
        even, odd = t._infer_variants(x)
        if cbcr is None:
            return ops.dihedral_merge_u8(even, odd)
        cbcr = ops.resize_u8(cbcr, int(even.shape[-2]), int(even.shape[-1]))
        return ops.dihedral_merge_u8(even, odd, cbcr[0], cbcr[1])
    out = t._infer(x)
    out = out[-1] if isinstance(out, tuple) else out
    if cbcr is None:
        return ops.to_u8_image(out)
    cbcr = ops.resize_u8(cbcr, int(out.shape[-2]), int(out.shape[-1]))
    return ops.ycbcr_to_rgb_u8(out, cbcr[0], cbcr[1])


def whole(model, which):
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import main as cli
    import tempfile
    from pytorch_super_resolution_model_collection_amd import tiling
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    nc = 3 if model == "EDSR" else 1
    args = cli.parse_args(["--model_name", model, "--num_channels", str(nc), "--scale_factor", str(SCALE), "--synthetic",
                           "--save_dir", tempfile.mkdtemp()])
    torch.manual_seed(1)
    t = TRAINERS[model](args)
    t.model = t.build_model()
    t.model.weight_init()
    t.model.to(t.device).eval()
    g = torch.Generator().manual_seed(7)
    geo = tiling.net_geometry(t.model)
    for size in which:
        h, w = SIZES[size]
        x = torch.rand((1, nc, h, w), generator=g).to(t.device)
        for tile in (None, TILE):
            label = "one pass" if tile is None else "tile %d" % tile
            if tile is None and tiling.resolve_tile("auto", geo, h, w) is not None:
                print("%s x%d %dx%d %s: not run, the widest activation (%.1f GB) is past the one-pass limit of the fast kernels"
                      % (model, SCALE, w, h, label, tiling.activation_bytes(geo, h, w) / 2 ** 30), flush=True)
                continue
            rgb = (x[0] if nc == 3 else x[0].expand(3, h, w)).permute(1, 2, 0).mul(255).to(torch.uint8).contiguous()
            forms = (("tensor form", lambda: t._forward(x, tile), lambda: t._forward(x, tile, self_ensemble=True)),
                     ("path form  ", lambda: _path_device(t, rgb, tile, False), lambda: _path_device(t, rgb, tile, True)))
            for form, single, ens in forms:
                res = {"single": [], "ensemble": []}
                for _ in range(5):   # five alternating rounds, three timings each
                    res["single"].append(_events(single, reps=3, warm=1)[0])
                    res["ensemble"].append(_events(ens, reps=3, warm=1)[0])
                s, e = statistics.median(res["single"]), statistics.median(res["ensemble"])
                print("%s x%d %dx%d %-9s %s single %9.3f ms, x 8 = %9.3f ms; ensemble call %9.3f ms; %+6.2f %% against the eight "
                      "singles" % (model, SCALE, w, h, label, form, s, 8 * s, e, (e / (8 * s) - 1) * 100), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "kernels":
        kernels(sys.argv[2:] or ["small", "large"])
    elif mode == "whole":
        whole(sys.argv[2], sys.argv[3:] or ["small", "large"])
