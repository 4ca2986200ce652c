#!/usr/bin/env python3
"""Evidence for DESIGN 32 (Real-ESRGAN's second-order degradation and USM targets), run on the MI355X box from the repo root:

  python tools/time_degrade2.py kernel          srk_noise2_u8 (Gaussian and Poisson, colour and gray), srk_usm_u8 and the BOX
                                                filter of srk_img_resize_u8 at [16, 3, 128, 128] and at the chain's small size
                                                [16, 3, 32, 32], each beside a torch composition of the same arithmetic (torch.randn
                                                / torch.poisson for the draws, fp64 separable conv2d on a reflect-padded input,
                                                adaptive_avg_pool2d) that exists in this tool only
  python tools/time_degrade2.py loader [sides]  patches/s of the resident-image loader (tools/loader_bench.py's set-up) at
                                                batch 16 and 64, crop 128
  python tools/time_degrade2.py host            host time of Degradation2.draw(batch): the draws and the tables, no device
  python tools/time_degrade2.py trainer [sides] ms per iteration of the EDSR trainer at batch 16 (tools/trainer_rate.py's
                                                set-up, replayed step)

sides: `both` (default: flags off, --degrade, --degrade2, --degrade2 --usm, alternated) or `off` (no degradation is ever
named, so the same file also runs on a tree from before the feature).  HIP events for the kernels, a host clock around a
device synchronise for the loader and the trainer; five alternating rounds, reported as min .. median .. max."""
import contextlib
import io
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = 5


def _events(fn, inner, warm=3):
    """us per call: `inner` calls between two events"""
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner * 1e3


def _alternate(sides, measure):
    """{name: thing} -> {name: [one figure per round]}, the sides alternated within every round"""
    res = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for name, thing in sides.items():
            res[name].append(measure(thing))
    return res


def _fmt(v, unit):
    return "%.4g .. %.4g .. %.4g %s (spread %.1f %%)" % (min(v), statistics.median(v), max(v), unit,
                                                       (max(v) - min(v)) / statistics.median(v) * 100)


def _row(what, r, unit="us"):
    a, b = statistics.median(r["srk"]), statistics.median(r["torch"])
    print("%s: srk %s | torch composition %s | torch / srk %.2f%s"
          % (what, _fmt(r["srk"], unit), _fmt(r["torch"], unit), b / a, "  ** the kernel loses **" if b < a else ""), flush=True)


def kernel():
    import torch
    import torch.nn.functional as F
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    ops = pkg.ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(3)
    cdf = torch.from_numpy(ops.poisson_cdf()).to(dev)
    g = torch.from_numpy(ops.usm_table()).to(dev)
    for B, C, H, W in ((16, 3, 128, 128), (16, 3, 32, 32)):
        x = torch.randint(0, 256, (B, C, H, W), generator=gen, dtype=torch.uint8).to(dev)
        amount = torch.linspace(1.0, 25.0, B, dtype=torch.float64).to(dev)
        scale = torch.linspace(0.05, 3.0, B, dtype=torch.float64).to(dev)
        one, zero = torch.ones(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
        shape = "[%d, %d, %d, %d]" % (B, C, H, W)

        def gauss(gray):
            z = torch.randn((B, 1 if gray else C, H, W), dtype=torch.float64, device=dev)
            return (x.double() + amount.view(B, 1, 1, 1) * z + 0.5).floor_().clamp_(0, 255).to(torch.uint8)

        def poisson(gray):
            level = (x.double().sum(1, keepdim=True) / 3.0 + 0.5).floor_() if gray else x.double()
            d = torch.poisson(level * (256.0 / 255.0)) * (255.0 / 256.0) - level
            return (x.double() + scale.view(B, 1, 1, 1) * d + 0.5).floor_().clamp_(0, 255).to(torch.uint8)

        for name, mode, amt, comp in (("Gaussian", one, amount, gauss), ("Poisson", 2 * one, scale, poisson)):
            for gray in (False, True):
                r = _alternate({"srk": lambda: ops.noise2_u8(x, mode, one if gray else zero, amt, cdf, 12345, 1),
                                "torch": lambda: comp(gray)}, lambda fn: _events(fn, 100))
                _row("noise2 %s %s %s" % (shape, name, "gray" if gray else "colour"), r)

        if H > 25:
            K = g.numel()
            gr, gc = g.view(1, 1, 1, K).repeat(B * C, 1, 1, 1), g.view(1, 1, K, 1).repeat(B * C, 1, 1, 1)

            def blur(a):
                p = F.pad(a.view(1, B * C, H, W), (K // 2,) * 4, mode="reflect")
                return F.conv2d(F.conv2d(p, gr, groups=B * C), gc, groups=B * C).view(B, C, H, W)

            def usm():
                p = x.double()
                res = p - blur(p)
                soft = blur((res.abs() > 10.0).double())
                sharp = (p + 0.5 * res).clamp_(0, 255)
                return ((soft * sharp + (1 - soft) * p).clamp_(0, 255) + 0.5).floor_().to(torch.uint8)

            diff = int((ops.usm_u8(x, g).int() - usm().int()).abs().max())
            r = _alternate({"srk": lambda: ops.usm_u8(x, g), "torch": usm}, lambda fn: _events(fn, 50))
            _row("usm %s K = %d (max |difference| %d level)" % (shape, K, diff), r)

        for oh in ((86, 32, 160) if H == 128 else (24, 9, 40)):
            planes = x.view(B * C, H, W)

            def area():
                y = F.adaptive_avg_pool2d(planes.float().unsqueeze(0), (oh, oh)) if oh < H else \
                    F.interpolate(planes.float().unsqueeze(0), size=(oh, oh), mode="nearest")
                return (y + 0.5).floor_().to(torch.uint8)

            r = _alternate({"srk": lambda: ops.resize_u8(planes, oh, oh, interpolation="box"), "torch": area},
                           lambda fn: _events(fn, 100))
            _row("BOX resize %s -> %d x %d" % (shape, oh, oh), r)
    torch.cuda.synchronize()


def host():
    import random
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    deg = pkg.data.Degradation2()
    random.seed(0)
    for batch in (16, 64):
        def once(_):
            t0 = time.perf_counter()
            for _ in range(50):
                deg.draw(batch)
            return (time.perf_counter() - t0) / 50 * 1e6
        once(None)
        print("Degradation2.draw(%d), host only: %s" % (batch, _fmt([once(None) for _ in range(ROUNDS)], "us")), flush=True)


def _png_folder(root, n, size=256):
    import numpy as np
    from PIL import Image
    d = os.path.join(root, "DIV2K", "DIV2K_train_LR_bicubic", "X4")
    os.makedirs(d)
    rng = np.random.RandomState(0)
    for i in range(n):
        Image.fromarray(rng.randint(0, 256, (size, size, 3), dtype=np.uint8)).save(os.path.join(d, "%04d.png" % i))


SIDES = ("off", "--degrade", "--degrade2", "--degrade2 --usm")


def _sides(which):
    if which not in ("both", "off"):
        raise SystemExit("sides: both | off")
    return SIDES if which == "both" else ("off",)


def loader(which="both"):
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    dev = torch.device("cuda", 0)
    n = 256
    with tempfile.TemporaryDirectory() as root:
        _png_folder(root, n)
        for batch in (16, 64):
            loaders = {}
            for side in _sides(which):
                kw = {}
                if side == "--degrade":
                    kw = dict(degrade=pkg.data.Degradation())
                elif side.startswith("--degrade2"):
                    kw = dict(degrade=pkg.data.Degradation2(), usm=side.endswith("--usm"))
                ds = pkg.data.get_training_set(root, ["DIV2K"], 128, 4, device=dev, **kw)
                loaders[side] = pkg.data.PatchLoader(ds, batch_size=batch, shuffle=True, num_threads=8, seed=1)
                for _ in loaders[side]:      # warm-up epoch: decode, upload (the images stay resident), kernels
                    pass

            def rate(ld):
                torch.cuda.synchronize()
                t0, k = time.perf_counter(), 0
                for _ in range(20):
                    for lr, hr, bc in ld:
                        k += lr.shape[0]
                torch.cuda.synchronize()
                return k / (time.perf_counter() - t0)

            r = _alternate(loaders, rate)
            print("loader, batch %d, crop 128, %d resident images: %s" % (batch, n, " | ".join(
                "%s %s" % (s, _fmt(v, "patches/s")) for s, v in r.items())), flush=True)


def trainer(which="both"):
    import torch
    import main as cli
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    n, batch, epochs = 256, 16, 8
    with tempfile.TemporaryDirectory() as root:
        _png_folder(root, n)
        runs = {}
        for side in _sides(which):
            args = cli.parse_args(["--model_name", "EDSR", "--num_epochs", "1", "--save_epochs", "100", "--batch_size",
                                   str(batch), "--crop_size", "128", "--data_dir", root, "--num_threads", "8",
                                   "--save_dir", os.path.join(root, "out_%d" % len(runs))] + ([] if side == "off" else side.split()))
            t = TRAINERS["EDSR"](args)
            ld = t.load_dataset(t.train_dataset, is_train=True)
            with contextlib.redirect_stdout(io.StringIO()):
                t.train(ld)                      # epoch 1: decode + upload, eager first step, capture
            t.num_epochs = epochs
            runs[side] = (t, ld)

        def ms_per_iteration(run):
            t, ld = run
            with contextlib.redirect_stdout(io.StringIO()):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                t.train(ld)                      # (re-initialises the model; the images stay resident)
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) / (epochs * len(ld)) * 1e3

        r = _alternate(runs, ms_per_iteration)
        print("EDSR trainer, batch %d, %d resident images, replayed step, %d iterations a round incl. model set-up: %s"
              % (batch, n, epochs * (n // batch), " | ".join("%s %s" % (s, _fmt(v, "ms / iteration")) for s, v in r.items())),
              flush=True)


if __name__ == "__main__":
    {"kernel": kernel, "host": host, "loader": loader, "trainer": trainer}[sys.argv[1] if len(sys.argv) > 1 else "kernel"](*sys.argv[2:3])
