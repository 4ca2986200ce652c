#!/usr/bin/env python3
"""Evidence for DESIGN 23 (the training degradations), run on the MI355X box from the repo root:

  python tools/time_degrade.py kernel          srk_blur_u8 at [16, 3, 128, 128] for K = 21 and K = 7 and srk_noise_u8 at
                                               [16, 3, 32, 32] and [64, 3, 32, 32], each beside a torch composition of the same
                                               arithmetic (fp64 depthwise conv2d on a reflect-padded input; torch.randn for the
                                               normals) that exists in this tool only
  python tools/time_degrade.py loader [sides]  patches/s of the resident-image loader (tools/loader_bench.py's set-up) at
                                               batch 16 and 64, crop 128
  python tools/time_degrade.py host            host time of Degradation.draw(batch): the draws and the tables, no device
  python tools/time_degrade.py trainer [sides] ms per iteration of the EDSR trainer at batch 16 (tools/trainer_rate.py's
                                               set-up, replayed step)

sides: `both` (default: the loader with degrade=None and with the default Degradation, alternated; the trainer also with
`--degrade --blur_prob 0`, which keeps the draws, the copy and the noise but launches no blur) or `off` (degrade is never
named, so the same file also runs on a tree from before the feature).  HIP events for the kernels, a host clock around
a device synchronise for the loader and the trainer; five alternating rounds, reported as min .. median .. max."""
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


def kernel():
    import numpy as np
    import torch
    import torch.nn.functional as F
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(3)
    rs = np.random.RandomState(3)
    for K, s_hi in ((21, 4.0), (7, 1.0)):
        B, C, H, W = 16, 3, 128, 128
        x = torch.randint(0, 256, (B, C, H, W), generator=gen, dtype=torch.uint8).to(dev)
        w = torch.from_numpy(np.stack([pkg.data.blur_weights(rs.uniform(0.8 * s_hi, s_hi), rs.uniform(0.2, s_hi),
                                                             rs.uniform(0, np.pi), K) for _ in range(B)])).to(dev)
        wk = w.repeat_interleave(C, 0).unsqueeze(1)          # [B * C, 1, K, K]: one group per plane

        def composed():
            p = F.pad(x.double().view(1, B * C, H, W), (K // 2,) * 4, mode="reflect")
            return (F.conv2d(p, wk, groups=B * C).clamp_(0, 255) + 0.5).floor_().to(torch.uint8).view(B, C, H, W)

        y = pkg.ops.blur_u8(x, w)
        diff = int((y.int() - composed().int()).abs().max())   # (the composition sums in another order: a level at most)
        r = _alternate({"srk": lambda: pkg.ops.blur_u8(x, w), "torch": composed}, lambda fn: _events(fn, 50))
        fma = B * C * H * W * K * K
        a, b = statistics.median(r["srk"]), statistics.median(r["torch"])
        print("blur  [%d, %d, %d, %d] K = %2d: srk_blur_u8 %s = %.2f T fp64 FMA/s | torch composition %s | torch / srk %.2f | "
              "max |difference| %d level" % (B, C, H, W, K, _fmt(r["srk"], "us"), fma / a / 1e6, _fmt(r["torch"], "us"), b / a,
                                             diff), flush=True)
    for B in (16, 64):
        x = torch.randint(0, 256, (B, 3, 32, 32), generator=gen, dtype=torch.uint8).to(dev)
        sigma = torch.linspace(1.0, 10.0, B, dtype=torch.float64).to(dev)

        def composed():
            z = torch.randn(x.shape, dtype=torch.float64, device=dev)
            return ((x.double() + sigma.view(B, 1, 1, 1) * z + 0.5).floor_().clamp_(0, 255).float() / 255.0)

        r = _alternate({"srk": lambda: pkg.ops.noise_u8(x, sigma, 12345), "torch": composed}, lambda fn: _events(fn, 200))
        a, b = statistics.median(r["srk"]), statistics.median(r["torch"])
        print("noise [%d, 3, 32, 32]: srk_noise_u8 %s | torch composition %s | torch / srk %.2f"
              % (B, _fmt(r["srk"], "us"), _fmt(r["torch"], "us"), b / a), flush=True)
    torch.cuda.synchronize()


def host():
    import random
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    deg = pkg.data.Degradation()
    random.seed(0)
    for batch in (16, 64):
        def once(_):
            t0 = time.perf_counter()
            for _ in range(200):
                deg.draw(batch)
            return (time.perf_counter() - t0) / 200 * 1e6
        once(None)
        print("Degradation.draw(%d), host only: %s" % (batch, _fmt([once(None) for _ in range(ROUNDS)], "us")), flush=True)


def _png_folder(root, n, size=256):
    import numpy as np
    from PIL import Image
    d = os.path.join(root, "DIV2K", "DIV2K_train_LR_bicubic", "X4")
    os.makedirs(d)
    rng = np.random.RandomState(0)
    for i in range(n):
        Image.fromarray(rng.randint(0, 256, (size, size, 3), dtype=np.uint8)).save(os.path.join(d, "%04d.png" % i))


def _sides(which):
    if which not in ("both", "off"):
        raise SystemExit("sides: both | off")
    return ("off", "on") if which == "both" else ("off",)


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
                kw = dict(degrade=pkg.data.Degradation()) if side == "on" else {}
                ds = pkg.data.get_training_set(root, ["DIV2K"], 128, 4, device=dev, **kw)
                loaders[side] = pkg.data.PatchLoader(ds, batch_size=batch, shuffle=True, num_threads=8, seed=1)
                for _ in loaders[side]:      # warm-up epoch: decode, upload (the images stay resident), kernels
                    pass

            def rate(ld):
                torch.cuda.synchronize()
                t0, k = time.perf_counter(), 0
                for _ in range(40):
                    for lr, hr, bc in ld:
                        k += lr.shape[0]
                torch.cuda.synchronize()
                return k / (time.perf_counter() - t0)

            r = _alternate(loaders, rate)
            print("loader, batch %d, crop 128, %d resident images: %s" % (batch, n, " | ".join(
                "degrade %s %s" % (s, _fmt(v, "patches/s")) for s, v in r.items())), flush=True)


def trainer(which="both"):
    import torch
    import main as cli
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    n, batch, epochs = 256, 16, 16
    with tempfile.TemporaryDirectory() as root:
        _png_folder(root, n)
        runs = {}
        flags = {"off": [], "on": ["--degrade"], "on, --blur_prob 0": ["--degrade", "--blur_prob", "0"]}
        for side in _sides(which) + (("on, --blur_prob 0",) if which == "both" else ()):
            args = cli.parse_args(["--model_name", "EDSR", "--num_epochs", "1", "--save_epochs", "100", "--batch_size",
                                   str(batch), "--crop_size", "128", "--data_dir", root, "--num_threads", "8",
                                   "--save_dir", os.path.join(root, "out_%d" % len(runs))] + flags[side])
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
              % (batch, n, epochs * (n // batch), " | ".join("--degrade %s %s" % (s, _fmt(v, "ms / iteration"))
                                                             for s, v in r.items())), flush=True)


if __name__ == "__main__":
    {"kernel": kernel, "host": host, "loader": loader, "trainer": trainer}[sys.argv[1] if len(sys.argv) > 1 else "kernel"](*sys.argv[2:3])
