#!/usr/bin/env python3
"""Evidence for DESIGN 24 (the JPEG stage of the training degradations), run on the MI355X box from the repo root:

  python tools/time_jpeg.py kernel           srk_jpeg_u8 at [16, 3, 32, 32] and [64, 3, 32, 32] (the training call) and at
                                             [1, 3, 339, 510] (the x4 LR of a 2040 x 1356 picture), 4:2:0 and 4:4:4, each
                                             as the loader calls it and through ops.jpeg_u8, beside what a user has without
                                             it -- device -> host, Pillow's save and open per patch, host -> device -- which
                                             exists in this tool only
  python tools/time_jpeg.py loader [sides]   patches/s of the resident-image loader (tools/time_degrade.py's set-up) at
                                             batch 16 and 64, crop 128
  python tools/time_jpeg.py trainer [sides]  ms per iteration of the EDSR trainer at batch 16 (the same set-up, replayed step)

sides: `all` (default: degrade=None, the default Degradation, and the same with jpeg_quality=(30, 95), alternated) or `off`
(neither is named, so the same file also runs on a tree from before the feature).  HIP events for the kernels, a host
clock around a device synchronise for the Pillow path, the loader and the trainer; five alternating rounds, reported as
min .. median .. max."""
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
HBM_BYTES_PER_S = 8.0e12     # MI355X peak HBM3E bandwidth


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


def _host_clock(fn, inner, warm=1):
    """us per call by the host's clock around a device synchronise"""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e6


def _alternate(sides, measure):
    """{name: thing} -> {name: [one figure per round]}, the sides alternated within every round"""
    res = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for name, thing in sides.items():
            res[name].append(measure(name, thing))
    return res


def _fmt(v, unit):
    return "%.4g .. %.4g .. %.4g %s (spread %.1f %%)" % (min(v), statistics.median(v), max(v), unit,
                                                       (max(v) - min(v)) / statistics.median(v) * 100)


def kernel():
    import numpy as np
    import torch
    from PIL import Image
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    from pytorch_super_resolution_model_collection_amd._lib import check, ptr
    lib = pkg._lib.load()
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(3)
    for (B, H, W), inner in (((16, 32, 32), 200), ((64, 32, 32), 200), ((1, 339, 510), 100)):
        # smooth content with some noise: what a shrunk photograph looks like to the coder
        yy, xx = np.mgrid[0:H, 0:W]
        base = 120.0 + 60.0 * np.sin(xx / 9.0) * np.cos(yy / 7.0)
        x_host = np.clip(base[None, None] + rs.normal(0, 12, (B, 3, H, W)), 0, 255).astype(np.uint8)
        x = torch.from_numpy(x_host).to(dev)
        q_host = rs.randint(30, 96, B)
        q = torch.from_numpy(q_host).to(dev)
        for sub, pil_sub in (("4:2:0", 2), ("4:4:4", 0)):
            def pillow():
                hwc = x.permute(0, 2, 3, 1).contiguous().cpu().numpy()
                out = np.empty_like(hwc)
                for b in range(B):
                    buf = io.BytesIO()
                    Image.fromarray(hwc[b], "RGB").save(buf, format="JPEG", quality=int(q_host[b]), subsampling=pil_sub)
                    out[b] = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
                return torch.from_numpy(out).to(dev).permute(0, 3, 1, 2).float().div_(255.0)

            q64, code, sp = q.double(), pkg.ops.jpeg_subsampling(sub), pkg.ops.stream_ptr()

            def srk():      # the loader's call (data._Device.jpeg): the result's allocation and the ctypes hand-over
                y = torch.empty(x.shape, dtype=torch.float32, device=dev)
                check(lib.srk_jpeg_u8(ptr(x), ptr(y), ptr(q64), 3, B, H, W, code, 1, 1, sp), "srk_jpeg_u8")
                return y

            op = lambda: pkg.ops.jpeg_u8(x, q, subsampling=sub, out_float=True)    # + the qualities' int -> fp64 cast
            differ = int((pkg.ops.jpeg_u8(x, q, subsampling=sub) != (pillow() * 255.0).round().to(torch.uint8)).sum())
            assert torch.equal(srk(), op())
            r = _alternate({"srk": (srk, inner), "op": (op, inner), "pillow": (pillow, 10)},
                           lambda name, t: (_host_clock if name == "pillow" else _events)(t[0], t[1]))
            a, b = statistics.median(r["srk"]), statistics.median(r["pillow"])
            moved = B * 3 * H * W * (1 + 4)           # bytes the call must move: 8-bit in, fp32 out
            print("jpeg [%d, 3, %d, %d] %s: srk_jpeg_u8 %s = %.3g GB/s in + out (%.2f %% of the %.0f TB/s HBM peak) | "
                  "ops.jpeg_u8 %s | d2h + Pillow + h2d %s | Pillow / srk %.0f | %d bytes differ"
                  % (B, H, W, sub, _fmt(r["srk"], "us"), moved / a / 1e3, moved / (a * 1e-6) / HBM_BYTES_PER_S * 100,
                     HBM_BYTES_PER_S / 1e12, _fmt(r["op"], "us"), _fmt(r["pillow"], "us"), b / a, differ), flush=True)
    torch.cuda.synchronize()


def _png_folder(root, n, size=256):
    import numpy as np
    from PIL import Image
    d = os.path.join(root, "DIV2K", "DIV2K_train_LR_bicubic", "X4")
    os.makedirs(d)
    rng = np.random.RandomState(0)
    for i in range(n):
        Image.fromarray(rng.randint(0, 256, (size, size, 3), dtype=np.uint8)).save(os.path.join(d, "%04d.png" % i))


def _sides(which):
    if which not in ("all", "off"):
        raise SystemExit("sides: all | off")
    return ("off", "degrade", "degrade + jpeg") if which == "all" else ("off",)


def loader(which="all"):
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
                if side != "off":
                    kw = dict(degrade=pkg.data.Degradation(**(dict(jpeg_quality=(30, 95)) if "jpeg" in side else {})))
                ds = pkg.data.get_training_set(root, ["DIV2K"], 128, 4, device=dev, **kw)
                loaders[side] = pkg.data.PatchLoader(ds, batch_size=batch, shuffle=True, num_threads=8, seed=1)
                for _ in loaders[side]:      # warm-up epoch: decode, upload (the images stay resident), kernels
                    pass

            def rate(_, ld):
                torch.cuda.synchronize()
                t0, k = time.perf_counter(), 0
                for _ in range(40):
                    for lr, hr, bc in ld:
                        k += lr.shape[0]
                torch.cuda.synchronize()
                return k / (time.perf_counter() - t0)

            r = _alternate(loaders, rate)
            print("loader, batch %d, crop 128, %d resident images: %s" % (batch, n, " | ".join(
                "%s %s" % (s, _fmt(v, "patches/s")) for s, v in r.items())), flush=True)


def trainer(which="all"):
    import torch
    import main as cli
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    n, batch, epochs = 256, 16, 16
    with tempfile.TemporaryDirectory() as root:
        _png_folder(root, n)
        runs = {}
        flags = {"off": [], "degrade": ["--degrade"], "degrade + jpeg": ["--degrade", "--jpeg_quality", "30,95"]}
        for side in _sides(which):
            args = cli.parse_args(["--model_name", "EDSR", "--num_epochs", "1", "--save_epochs", "100", "--batch_size",
                                   str(batch), "--crop_size", "128", "--data_dir", root, "--num_threads", "8",
                                   "--save_dir", os.path.join(root, "out_%d" % len(runs))] + flags[side])
            t = TRAINERS["EDSR"](args)
            ld = t.load_dataset(t.train_dataset, is_train=True)
            with contextlib.redirect_stdout(io.StringIO()):
                t.train(ld)                      # epoch 1: decode + upload, eager first step, capture
            t.num_epochs = epochs
            runs[side] = (t, ld)

        def ms_per_iteration(_, run):
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
    {"kernel": kernel, "loader": loader, "trainer": trainer}[sys.argv[1] if len(sys.argv) > 1 else "kernel"](*sys.argv[2:3])
