#!/usr/bin/env python3
"""Evidence for DESIGN 16 (the picture-file tail of test_single), run on the MI355X box from the repo root:

  python tools/test_single_profile.py prepare DIR          a seeded 510 x 339 picture and freshly initialised VDSR (Y) and
                                                           EDSR (RGB) checkpoints under DIR, where main.py looks for them
  rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d OUT/vdsr -o vdsr -- \\
      python main.py --model_name VDSR --num_channels 1 --save_dir DIR --test_single DIR/picture.png
  rocprofv3 ... -d OUT/vdsr_x5 -o vdsr_x5 -- python tools/test_single_profile.py run VDSR DIR 5      (warm launches)
  rocprofv3 ... -d OUT/edsr_x5 -o edsr_x5 -- python tools/test_single_profile.py run EDSR DIR 5
  python tools/test_single_profile.py pillow DIR           the same tail with Pillow on the host CPU
  python tools/test_single_profile.py summarize OUT/vdsr [OUT/vdsr_x5 ...]     -> text for profiles/

`summarize` orders kernels and copies of a trace by start time, cuts it into test_single calls at k_rgb_to_ycc (Y
models) or at the host-to-device upload before k_to_u8 (RGB models), and prints for every call the kernels of the tail
with their durations, what was copied between the upload and the last kernel, and the copies after it."""
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, SCALE = 510, 339, 4


def _args(model, d):
    import main as cli
    return cli.parse_args(["--model_name", model, "--num_channels", "1" if model == "VDSR" else "3", "--scale_factor", str(SCALE),
                           "--save_dir", d, "--synthetic"])


def prepare(d):
    import numpy as np
    import torch
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    rs = np.random.RandomState(5)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([xx / W, yy / H, 0.5 + 0.5 * np.sin(xx / 31.0) * np.cos(yy / 23.0)], axis=-1)
    Image.fromarray(np.clip(base * 255 + rs.normal(0, 12, size=(H, W, 3)), 0, 255).astype(np.uint8), "RGB").save(os.path.join(d, "picture.png"))
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    for model in ("VDSR", "EDSR"):
        torch.manual_seed(1)
        t = TRAINERS[model](_args(model, d))
        t.model = t.build_model()
        t.model.weight_init()
        t.save_model()


def run(model, d, n):
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    t = TRAINERS[model](_args(model, d))
    for _ in range(n):
        print(t.test_single(os.path.join(d, "picture.png")))


def pillow(d, reps=20):
    from PIL import Image
    img = Image.open(os.path.join(d, "picture.png")).convert("RGB")
    size = (W * SCALE, H * SCALE)
    recon_y = img.convert("L").resize(size, Image.BICUBIC)      # stands for the net's quantised Y output (not timed)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        y, cb, cr = img.convert("YCbCr").split()
        out = Image.merge("YCbCr", [recon_y, cb.resize(size, Image.BICUBIC), cr.resize(size, Image.BICUBIC)]).convert("RGB")
        times.append(time.perf_counter() - t0)
    times.sort()
    print("Pillow %s tail on the host CPU (convert, split, two bicubic resizes %dx%d -> %dx%d, merge, convert): "
          "median %.3f ms, min %.3f ms over %d runs" % (Image.__version__, W, H, size[0], size[1], times[len(times) // 2] * 1e3,
                                                        times[0] * 1e3, reps))
    return out


def _rows(d, suffix):
    hits = glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)
    if not hits:
        return []
    with open(hits[0]) as fh:
        return list(csv.DictReader(fh))


def summarize(d):
    ev = []
    for r in _rows(d, "kernel_trace.csv"):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "K", r["Kernel_Name"].split("(")[0].replace("void ", "").replace("srk::", "")))
    for r in _rows(d, "memory_copy_trace.csv"):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "C", r.get("Direction", "?").replace("MEMORY_COPY_", "")))
    ev.sort()
    print("== %s: %d kernels, %d copies" % (os.path.basename(d.rstrip("/")), sum(e[2] == "K" for e in ev), sum(e[2] == "C" for e in ev)))
    is_tail = lambda e: e[2] == "K" and (e[3].startswith("k_ycc_to_rgb") or e[3].startswith("k_to_u8"))
    ends = [i for i, e in enumerate(ev) if is_tail(e)]
    prev = -1
    for call, last in enumerate(ends):
        # the call's upload: the last host-to-device copy before its first colour kernel / before the net
        head = "k_rgb_to_ycc" if ev[last][3].startswith("k_ycc_to_rgb") else "k_copy_u8_strided"   # RGB: ToTensor's first kernel
        first = max([i for i in range(prev + 1, last) if ev[i][2] == "K" and ev[i][3].startswith(head)] or [prev + 1])
        h2d = [i for i in range(prev + 1, first + 1) if ev[i][2] == "C" and "HOST_TO_DEVICE" in ev[i][3]]
        start = h2d[-1] if h2d else first
        nxt = ends[call + 1] if call + 1 < len(ends) else len(ev)
        after = [ev[i] for i in range(last + 1, nxt) if ev[i][2] == "C" and "DEVICE_TO_HOST" in ev[i][3]]
        nxt_up = [i for i in range(last + 1, nxt) if ev[i][2] == "C" and "HOST_TO_DEVICE" in ev[i][3]]
        after = [e for e in after if not nxt_up or e[0] < ev[nxt_up[0]][0]]
        between = [ev[i] for i in range(start + 1, last) if ev[i][2] == "C"]
        tail = [ev[last]]
        i = last - 1
        while i > start and ev[i][2] == "K" and ev[last][3].startswith("k_ycc_to_rgb") \
                and ev[i][3] in ("k_resize_tables", "k_resize_h_u8", "k_resize_v_u8", "k_copy_u8_strided"):   # the two chroma resizes
            tail.insert(0, ev[i])
            i -= 1
        if ev[first][3].startswith("k_rgb_to_ycc"):
            tail.insert(0, ev[first])
        total = sum(e[1] - e[0] for e in tail)
        print("call %d: %d kernels between upload and last kernel, wall %.1f us; copies in between: %d %s; "
              "device-to-host copies after the last kernel: %d%s"
              % (call + 1, sum(e[2] == "K" for e in ev[start:last + 1]), (ev[last][1] - ev[start][0]) / 1e3, len(between),
                 sorted(set(e[3] for e in between)), len(after),
                 "".join(" (%.1f us)" % ((e[1] - e[0]) / 1e3) for e in after)))
        print("   tail kernels %.1f us: %s" % (total / 1e3, ", ".join("%s %.1f" % (e[3], (e[1] - e[0]) / 1e3) for e in tail)))
        prev = last
    stats = _rows(d, "kernel_stats.csv")
    for r in stats:
        n = r.get("Name", "")
        if any(k in n for k in ("k_rgb_to_ycc", "k_ycc_to_rgb", "k_to_u8", "k_resize_h_u8", "k_resize_v_u8", "k_resize_tables",
                                "k_u8_to_float", "k_copy_u8")):
            print("   stats %-60s calls %s avg %s ns min %s ns" % (n.split("(")[0], r.get("Calls"), r.get("AverageNs"), r.get("MinNs")))


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "prepare":
        prepare(sys.argv[2])
    elif mode == "run":
        run(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    elif mode == "pillow":
        pillow(sys.argv[2])
    elif mode == "summarize":
        for d in sys.argv[2:]:
            summarize(d)
