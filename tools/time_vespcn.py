#!/usr/bin/env python3
"""Times the motion-compensation operators against the torch compositions they replace and writes profiles/vespcn.txt.

  motion_fuse forward + backward   vs   grid build + two grid_sample + cat + mse_loss + autograd
  flow_huber_loss forward + backward   vs   slices, pad, sqrt, mean + autograd
at frames [16,3,1,32,32], [64,3,1,64,64], [8,3,3,270,480]; a replayed VESPCN x4 train step at batch 16, 32 x 32 LR against
the same net on the torch compositions; test_video frames/s against ESPCN.  --bench_log / --kernels_log quote the lines of
two runs made beside this one (bench.py on the parent commit and this tree in turn; the kernel names of a replayed EDSR
step under a kernel trace on both), so that a re-run keeps them.

Method: every candidate is captured as one hipGraph; a burst of REPS replays is timed with HIP events; the candidates
alternate over five rounds in one process; median and range of the per-replay times.  Bytes are the compulsory traffic
(frames read once forward and once backward, fused written, the flow read twice, dflow written, the fused gradient
read); the floor is that over HBM_GBS.

  python tools/time_vespcn.py [--out profiles/vespcn.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

HBM_GBS = 8000.0     # MI355X: 8 TB/s peak
ROUNDS, REPS = 5, 50
SHAPES = [(16, 1, 32, 32), (64, 1, 64, 64), (8, 3, 270, 480)]


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        fn()
    return g


def burst(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g.replay()
    a.record()
    for _ in range(REPS):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / REPS     # us


def compare(cands):
    graphs = [(name, graphed(fn)) for name, fn in cands]
    times = {name: [] for name, _ in graphs}
    for _ in range(ROUNDS):
        for name, g in graphs:
            times[name].append(burst(g))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def torch_warp(img, flow):
    n, c, h, w = img.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=img.device, dtype=img.dtype),
                            torch.arange(w, device=img.device, dtype=img.dtype), indexing="ij")
    gx = (xs[None] + flow[:, 0]) * (2.0 / max(w - 1, 1)) - 1.0
    gy = (ys[None] + flow[:, 1]) * (2.0 / max(h - 1, 1)) - 1.0
    return F.grid_sample(img, torch.stack([gx, gy], -1), mode="bilinear", padding_mode="border", align_corners=True)


def video_rates(dev):
    """test_video frames/s, ESPCN x4 (independent frames) against VESPCN x4 (three-frame windows), Y models, on
    tools/time_video.py's 480 x 270 4:2:0 stream of 64 frames at batch 8; whole calls, alternating rounds."""
    import io
    import tempfile
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import main as cli
    import video_ref as R
    from pytorch_super_resolution_model_collection_amd.sr_trainers import trainer_class
    frames_n, W, H = 64, 480, 270
    data = R.stream("W%d H%d F30:1 C420jpeg" % (W, H), R.random_frames(3, frames_n, W, H, "420"))
    nets = {}
    for name in ("ESPCN", "VESPCN"):
        t = trainer_class(name)(cli.parse_args(["--model_name", name, "--num_channels", "1", "--scale_factor", "4",
                                                "--save_dir", tempfile.mkdtemp()]))
        t.model = t.build_model().to(t.device).eval()
        t.test_video(io.BytesIO(data), io.BytesIO(), batch=8)       # warm
        nets[name] = t
    fps = {name: [] for name in nets}
    for _ in range(ROUNDS):
        for name, t in nets.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.test_video(io.BytesIO(data), io.BytesIO(), batch=8)
            fps[name].append(frames_n / (time.perf_counter() - t0))
    out = ["test_video, 480 x 270 4:2:0, 64 frames, batch 8, x4 Y models, frames/s (median, min .. max of %d calls):" % ROUNDS]
    for name, v in fps.items():
        out.append("  %-44s %9.1f (%.1f .. %.1f)" % (name, statistics.median(v), min(v), max(v)))
    return out + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vespcn.txt"))
    ap.add_argument("--bench_log", default=None, help="lines to quote: bench.py on the parent and this tree in turn")
    ap.add_argument("--kernels_log", default=None, help="lines to quote: the kernel-name comparison of a replayed EDSR step")
    args = ap.parse_args()
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd import models, ops, trainers
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = ["VESPCN's operators on one MI355X: replayed graphs, HIP events, %d alternating rounds of %d replays, median (min .. max) us"
             % (ROUNDS, REPS), ""]

    def row(name, r, floor=None):
        med, lo, hi = r
        tail = "" if floor is None else "  floor %.1f us = %.0f %% reached" % (floor, 100.0 * floor / med)
        lines.append("  %-44s %9.1f (%.1f .. %.1f)%s" % (name, med, lo, hi, tail))

    for n, c, h, w in SHAPES:
        frames = torch.rand(n, 3, c, h, w, device=dev)
        flow = ((torch.rand(2 * n, 2, h, w, device=dev) - 0.5) * 4).requires_grad_(True)
        g = torch.randn(n, 3 * c, h, w, device=dev).contiguous(memory_format=torch.channels_last)
        unit = ops.unit_seed(dev)

        def ours():
            fused, mc = ops.motion_fuse(frames, flow)
            torch.autograd.grad([fused, mc], [flow], [g, unit])

        def theirs():
            wa, wb = torch_warp(frames[:, 0], flow[:n]), torch_warp(frames[:, 2], flow[n:])
            fused = torch.cat([wa, frames[:, 1], wb], 1)
            mc = 0.5 * (F.mse_loss(wa, frames[:, 1]) + F.mse_loss(wb, frames[:, 1]))
            torch.autograd.grad([fused, mc], [flow], [g, unit])

        def hub_ours():
            torch.autograd.grad([ops.flow_huber_loss(flow)], [flow], [unit])

        def hub_theirs():
            dx = F.pad(flow[..., 1:] - flow[..., :-1], (0, 1))
            dy = F.pad(flow[..., 1:, :] - flow[..., :-1, :], (0, 0, 0, 1))
            torch.autograd.grad([torch.sqrt(0.01 + (dx ** 2).sum(1) + (dy ** 2).sum(1)).mean()], [flow], [unit])

        px = n * h * w
        fuse_bytes = 4 * (2 * 3 * c * px + 3 * c * px + 3 * c * px + 2 * 4 * px + 4 * px)
        hub_bytes = 4 * (2 * 4 * px + 4 * px)
        lines.append("frames [%d,3,%d,%d,%d], flow [%d,2,%d,%d]: %.2f MB / %.2f MB compulsory" % (n, c, h, w, 2 * n, h, w,
                                                                                                 fuse_bytes / 1e6, hub_bytes / 1e6))
        r = compare([("motion_fuse fwd+bwd (HIP)", ours), ("torch composition", theirs)])
        row("motion_fuse fwd+bwd (HIP)", r["motion_fuse fwd+bwd (HIP)"], fuse_bytes / (HBM_GBS * 1e3))
        row("grid_sample x2 + cat + mse + autograd", r["torch composition"])
        r = compare([("flow_huber fwd+bwd (HIP)", hub_ours), ("torch composition", hub_theirs)])
        row("flow_huber fwd+bwd (HIP)", r["flow_huber fwd+bwd (HIP)"], hub_bytes / (HBM_GBS * 1e3))
        row("slices + pad + sqrt + mean + autograd", r["torch composition"])
        lines.append("")

    # the replayed step: the net on the fused kernels against the SAME net (every conv on the library) with the three
    # operators swapped for their torch compositions
    batch = (torch.rand(16, 3, 3, 32, 32, device=dev), torch.rand(16, 3, 96, 96, device=dev))

    def torch_fuse(frames, flow):
        n = frames.shape[0]
        wa, wb = torch_warp(frames[:, 0], flow[:n]), torch_warp(frames[:, 2], flow[n:])
        return torch.cat([wa, frames[:, 1], wb], 1), 0.5 * (F.mse_loss(wa, frames[:, 1]) + F.mse_loss(wb, frames[:, 1]))

    def torch_huber(flow, eps=0.01):
        dx = F.pad(flow[..., 1:] - flow[..., :-1], (0, 1))
        dy = F.pad(flow[..., 1:, :] - flow[..., :-1, :], (0, 0, 0, 1))
        return torch.sqrt(eps + (dx ** 2).sum(1) + (dy ** 2).sum(1)).mean()

    def captured_step():
        torch.manual_seed(1)
        net = models.VESPCNNet(3, 64, 4).to(dev).train()
        net.weight_init()
        flat, opt, _, step = trainers.build("vespcn", net, 1e-4)
        return trainers.capture_step(step, batch, warmup=2, flats=[flat])

    hip_ops = (ops.motion_fuse, ops.flow_warp, ops.flow_huber_loss)
    gs_hip = captured_step()
    ops.motion_fuse, ops.flow_warp, ops.flow_huber_loss = torch_fuse, torch_warp, torch_huber
    try:
        gs_torch = captured_step()
    finally:
        ops.motion_fuse, ops.flow_warp, ops.flow_huber_loss = hip_ops
    times = {"hip": [], "torch": []}
    for _ in range(ROUNDS):
        for name, gs in (("hip", gs_hip), ("torch", gs_torch)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            gs(*batch)
            a.record()
            for _ in range(REPS):
                gs(*batch)
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) * 1000.0 / REPS)
    gs_hip.close()
    gs_torch.close()
    lines.append("replayed VESPCN x4 train step, batch 16, 32 x 32 LR, RGB (one graph each):")
    row("step on the fused kernels", (statistics.median(times["hip"]), min(times["hip"]), max(times["hip"])))
    row("same net on the torch compositions", (statistics.median(times["torch"]), min(times["torch"]), max(times["torch"])))
    lines.append("")
    lines += video_rates(dev)
    for title, path in (("bench.py --gpus 1 --steps 20 --warmup 5, the parent commit and this tree in turn on one box (images/s):",
                         args.bench_log), ("kernel names of a replayed EDSR step under a kernel trace, this tree against the "
                                           "parent commit:", args.kernels_log)):
        if path and os.path.exists(path):
            lines += [title] + ["  " + ln.rstrip() for ln in open(path)] + [""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
