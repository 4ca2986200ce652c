#!/usr/bin/env python3
"""Evidence for DESIGN 35 (raw video on the device), run from the repo root on the MI355X box:

  python tools/time_video.py [--quick]

1. ops.yuv_unpack and ops.yuv_pack (one launch each) at [64, 256 x 256] (4:2:0, Y model, x4 output) and [8, 960 x 540]
   (4:2:0, RGB model, x2 output), by HIP events around bursts of 50 back-to-back calls, beside the host time a call takes
   to enqueue (a row where that is the larger part is launch-bound: it does not show the kernel), warm, in five rounds
   that alternate with a torch composition of the same integer arithmetic on the device (table look-ups by index, shifts,
   the two-pass shrink).  "HBM floor" is the bytes the operator has to move -- every input byte read once, every output
   byte written once -- over 8 TB/s.
2. test_video as a whole, ESPCN (num_channels 1) x4 on a 480 x 270 stream and x2 on 960 x 540, source and sink in memory
   (BytesIO): frames a second by the host clock over the whole call, five rounds; the stages of one steady-state batch
   (upload, unpack, net, chroma, pack, download) by HIP events on their own; and what a user does without test_video: a
   loop of test_single(tensor) a frame with the chroma resized by Pillow on the host, on the same stream."""
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK, ROUNDS = 8e12, 5


BURST = 50


def _events(fn, reps):
    """us per call: the median over `reps` bursts of BURST back-to-back calls between two events.  A call whose kernel is
    shorter than the host's enqueue path (ctypes, checks, the allocator: about 10 us) still shows that path, not the kernel:
    such rows are launch-bound and say so."""
    import torch
    us = []
    for _ in range(max(1, reps // 4)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BURST):
            fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / BURST)
    return statistics.median(us)


def _host_us(fn, n=200):
    """us of host time a call takes to enqueue (no wait for the device inside the loop)."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return dt / n * 1e6


def color_tables(dev):
    """Pillow's fixed-point tables (csrc/color_common.h) as int32 device tensors."""
    import torch
    T = lambda c, lo: torch.tensor([int(c * 64 * i + 0.5) for i in range(lo, lo + 256)], dtype=torch.int32, device=dev)
    fwd = [T(c, 0) for c in (.299, .587, .114, -.16874, -.33126, -.41869, -.08131)]
    inv = [T(1.402, -128) >> 6, T(1.772, -128) >> 6, T(-.34414, -128), T(-.71414, -128), torch.full((), 255.0, device=dev)]
    return fwd, inv


def torch_unpack(frames, lay, channels, full, inv):
    import torch
    n, pix = frames.shape[0], lay.W * lay.H
    y = frames[:, :pix]
    if channels == 1:
        return (y.float() / inv[4]).view(n, 1, lay.H, lay.W)      # a tensor divisor: a scalar one becomes a multiplication
    yi, cb, cr = y.int(), full[0].reshape(n, pix).long(), full[1].reshape(n, pix).long()
    r = (yi + inv[0][cr]).clamp(0, 255)
    g = (yi + ((inv[2][cb] + inv[3][cr]) >> 6)).clamp(0, 255)
    b = (yi + inv[1][cb]).clamp(0, 255)
    return (torch.stack([r, g, b], 1).float() / inv[4]).view(n, 3, lay.H, lay.W)


def torch_pack(y, lay, chroma, fwd):
    import torch
    n = y.shape[0]
    q = (torch.nan_to_num(y, nan=0.0).clamp(0, 1) * 255.0).to(torch.uint8)
    if y.shape[1] == 1:
        return torch.cat([q.view(n, -1), chroma[0].reshape(n, -1), chroma[1].reshape(n, -1)], 1)
    r, g, b = (q[:, k].long() for k in range(3))
    yy = (fwd[0][r] + fwd[1][g] + fwd[2][b]) >> 6
    cb = ((fwd[3][r] + fwd[4][g] + 32 * b.int()) >> 6) + 128
    cr = ((32 * r.int() + fwd[5][g] + fwd[6][b]) >> 6) + 128

    def box(p):
        h = (p[:, :, 0::2] + p[:, :, 1::2] + 1) >> 1
        return (h[:, 0::2] + h[:, 1::2] + 1) >> 1
    return torch.cat([yy.view(n, -1), box(cb).reshape(n, -1), box(cr).reshape(n, -1)], 1).to(torch.uint8)


def kernels(pkg, dev, n, W, H, channels, scale):
    import numpy as np
    import torch
    ops = pkg.ops
    lay, out_lay = ops.yuv_layout(W, H, "420"), ops.yuv_layout(scale * W, scale * H, "420")
    fwd, inv = color_tables(dev)
    frames = torch.randint(0, 256, (n, lay.frame_bytes), dtype=torch.uint8, device=dev)
    full = ops.yuv_chroma(frames, lay, H, W) if channels == 3 else None
    y = torch.rand((n, channels, out_lay.H, out_lay.W), device=dev) * 1.2 - 0.1
    chroma = ops.yuv_chroma(frames, lay, out_lay.ch, out_lay.cw) if channels == 1 else None
    pix, opix = W * H, out_lay.W * out_lay.H
    need_un = n * pix * (1 if channels == 1 else 3) + 4 * n * channels * pix
    need_pk = 4 * n * channels * opix + (n * 2 * out_lay.cw * out_lay.ch if channels == 1 else 0) + n * out_lay.frame_bytes
    same = (torch.equal(ops.yuv_unpack(frames, lay, channels, full), torch_unpack(frames, lay, channels, full, inv)),
            torch.equal(ops.yuv_pack(y, out_lay, chroma), torch_pack(y, out_lay, chroma, fwd)))
    out_x = torch.empty((n, channels, H, W), device=dev)
    out_f = torch.empty((n, out_lay.frame_bytes), dtype=torch.uint8, device=dev)
    print("\n[%d, %d x %d] 4:2:0, %s model, x%d output; the torch compositions give the same bits: unpack %s, pack %s"
          % (n, W, H, "Y" if channels == 1 else "RGB", scale, same[0], same[1]))
    for name, need, fn, alt in (("yuv_unpack", need_un, lambda: ops.yuv_unpack(frames, lay, channels, full, out=out_x),
                                 lambda: torch_unpack(frames, lay, channels, full, inv)),
                                ("yuv_pack", need_pk, lambda: ops.yuv_pack(y, out_lay, chroma, out=out_f),
                                 lambda: torch_pack(y, out_lay, chroma, fwd))):
        kern, comp = [], []
        for _ in range(ROUNDS):
            kern.append(_events(fn, 20))
            comp.append(_events(alt, 5))
        km, cm = statistics.median(kern), statistics.median(comp)
        floor_us = need / PEAK * 1e6
        host = _host_us(fn)
        print("  ops.%-10s median %8.1f us a call (rounds %.1f .. %.1f; the host needs %.1f us to enqueue one%s)  %6.1f MB moved, "
              "%4.1f %% of the HBM floor's rate;  torch composition %8.1f us (rounds %.1f .. %.1f) = %.2fx%s"
              % (name, km, min(kern), max(kern), host, ": LAUNCH-BOUND, this is not the kernel's time" if host > 0.8 * km else "",
                 need / 1e6, 100 * floor_us / km, cm, min(comp), max(comp), cm / km,
                 "  **the kernel loses**" if cm < km else ""))


def whole_call(pkg, dev, W, H, scale, frames_n, batch):
    import numpy as np
    import torch
    import tempfile
    import main as cli
    import video_ref as R
    from PIL import Image
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    ops = pkg.ops
    t = TRAINERS["ESPCN"](cli.parse_args(["--model_name", "ESPCN", "--num_channels", "1", "--scale_factor", str(scale),
                                          "--save_dir", tempfile.mkdtemp()]))
    t.model = t.build_model().to(t.device).eval()
    lay = ops.yuv_layout(W, H, "420")
    data = R.stream("W%d H%d F30:1 C420jpeg" % (W, H), R.random_frames(3, frames_n, W, H, "420"))
    sink = io.BytesIO()
    t.test_video(io.BytesIO(data), sink, batch=batch)      # warm: plans, pinned buffers' first touch
    fps = []
    for _ in range(ROUNDS):
        sink = io.BytesIO()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.test_video(io.BytesIO(data), sink, batch=batch)
        fps.append(frames_n / (time.perf_counter() - t0))
    period_us = batch / statistics.median(fps) * 1e6
    # the stages of one steady-state batch, each alone on the stream
    pin = torch.from_numpy(R.random_frames(4, batch, W, H, "420")).pin_memory()
    dev_in = torch.empty(pin.shape, dtype=torch.uint8, device=dev)
    x = ops.yuv_unpack(dev_in.copy_(pin), lay, 1)
    y = t._net(t._net_input(x))
    out_lay = ops.yuv_layout(int(y.shape[-1]), int(y.shape[-2]), "420")
    chroma = ops.yuv_chroma(dev_in, lay, out_lay.ch, out_lay.cw)
    dev_out = ops.yuv_pack(y, out_lay, chroma)
    pin_out = torch.empty(dev_out.shape, dtype=torch.uint8, pin_memory=True)
    stages = (("upload", lambda: dev_in.copy_(pin, non_blocking=True)), ("unpack", lambda: ops.yuv_unpack(dev_in, lay, 1, out=x)),
              ("net", lambda: t._net(t._net_input(x))), ("chroma", lambda: ops.yuv_chroma(dev_in, lay, out_lay.ch, out_lay.cw)),
              ("pack", lambda: ops.yuv_pack(y, out_lay, chroma, out=dev_out)),
              ("download", lambda: pin_out.copy_(dev_out, non_blocking=True)))
    us = {name: statistics.median([_events(fn, 10) for _ in range(ROUNDS)]) for name, fn in stages}
    compute = us["unpack"] + us["net"] + us["chroma"] + us["pack"]
    longest = max(us["upload"], compute, us["download"])
    # without test_video: test_single(tensor) a frame, chroma by Pillow on the host
    few = min(frames_n, 12)
    payload = R.parse(data)[4][:few]

    def by_hand():
        out = []
        for f in payload:
            yy, cb, cr = R.planes(f, W, H, "420")
            sr = t.test_single(torch.from_numpy(yy.astype(np.float32) / np.float32(255.0)).view(1, 1, H, W))[0, 0].numpy()
            oh, ow = sr.shape
            out.append(b"FRAME\n" + R.quantise(sr).tobytes()
                       + Image.fromarray(cb).resize((ow // 2, oh // 2), Image.BICUBIC).tobytes()
                       + Image.fromarray(cr).resize((ow // 2, oh // 2), Image.BICUBIC).tobytes())
        return b"".join(out)
    mine = by_hand()
    same = mine == sink.getvalue()[sink.getvalue().index(b"\n") + 1:][:len(mine)]
    hand = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        by_hand()
        hand.append(few / (time.perf_counter() - t0))
    fm, hm = statistics.median(fps), statistics.median(hand)
    print("\nESPCN x%d (Y model) on %d frames of %d x %d 4:2:0 -> %d x %d, batch %d, BytesIO to BytesIO"
          % (scale, frames_n, W, H, out_lay.W, out_lay.H, batch))
    print("  test_video            %8.1f frames/s (rounds %.1f .. %.1f): a batch every %.0f us" % (fm, min(fps), max(fps), period_us))
    print("  one batch, stage by stage (us): " + ", ".join("%s %.0f" % (k, v) for k, v in us.items()))
    print("  streams: upload %.0f us, compute %.0f us, download %.0f us; the batch period is %.0f us over the longest (%.2fx)"
          % (us["upload"], compute, us["download"], period_us - longest, period_us / longest))
    print("  test_single per frame %8.1f frames/s (rounds %.1f .. %.1f), %s: test_video is %.1fx%s"
          % (hm, min(hand), max(hand), "the same bytes" if same else "NOT the same bytes (batch-of-one conv plans)", fm / hm,
             "" if fm > hm else "  **test_video does not win**"))


def main():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    quick = "--quick" in sys.argv
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(0))
    kernels(pkg, dev, 64, 256, 256, 1, 4)
    kernels(pkg, dev, 8, 960, 540, 3, 2)
    whole_call(pkg, dev, 480, 270, 4, 32 if quick else 96, 8)
    if not quick:
        whole_call(pkg, dev, 960, 540, 2, 64, 8)


if __name__ == "__main__":
    main()
