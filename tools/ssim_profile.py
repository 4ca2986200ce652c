#!/usr/bin/env python3
"""Evidence for DESIGN 18 (SSIM on the device), run from the repo root:

  python tools/ssim_profile.py time        on the MI355X box: k_ssim_partial + k_ssim_final (one srk_ssim call, workspace
                                           allocated once) on 1 x 2040 x 1356 (a Y plane) and on 3 x 2040 x 1356 with a
                                           channels-last prediction against an NCHW target, in the three domains: HIP
                                           events, warm, median of 30; beside srk_psnr on the same pair, and beside the
                                           route without the kernel (copy both tensors to the host, the fp64 restatement
                                           of tests/ssim_ref.py there)
  python tools/ssim_profile.py resources   anywhere hipcc is: registers, LDS and scratch of the two kernels from the
                                           compiler's resource report

"bytes needed" is 2 x 4 B per compared value; the share is of 8 TB/s."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
H, W, REPS, PEAK = 2040, 1356, 30, 8e12


def _events(fn, reps=REPS, warm=3):
    import torch
    for _ in range(warm):
        fn()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return statistics.median(us), min(us)


def timing():
    import numpy as np
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    from pytorch_super_resolution_model_collection_amd._lib import SSIM_DOMAINS, ptr, stream_ptr
    from pytorch_super_resolution_model_collection_amd.ops import _strides4
    import ssim_ref
    lib = pkg._lib.load()
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(0))
    ws = torch.empty(int(lib.srk_ssim_workspace_bytes()), dtype=torch.uint8, device=dev)
    ws_p = torch.empty(int(lib.srk_psnr_workspace_bytes()), dtype=torch.uint8, device=dev)
    out = torch.empty(3, device=dev)
    rng = np.random.RandomState(1)
    for c in (1, 3):
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        g = np.stack([0.5 + 0.4 * np.sin(xx / (11.0 + k)) * np.cos(yy / (17.0 + k)) for k in range(c)])[None]
        g = np.clip(g + 0.02 * rng.standard_normal(g.shape), 0, 1).astype(np.float32)
        p = (g + 0.04 * rng.standard_normal(g.shape)).astype(np.float32)
        pd = torch.from_numpy(p).to(dev).contiguous(memory_format=torch.channels_last)
        gd = torch.from_numpy(g).to(dev)
        need = 2 * 4 * c * H * W
        print("\n%d x %d x %d, prediction channels-last, target NCHW; bytes needed %.1f MB" % (c, H, W, need / 1e6))

        def psnr():
            lib.srk_psnr(ptr(pd), _strides4(pd), ptr(gd), _strides4(gd), 1, c, H, W, ptr(out[1:2]), ptr(out[2:3]), ptr(ws_p),
                         stream_ptr())
        med, lo = _events(psnr)
        print("  srk_psnr                      median %8.1f us  min %8.1f us  %5.1f %% of 8 TB/s" % (med, lo, 100 * need / (med * 1e-6) / PEAK))
        for domain in ("float", "u8", "y8"):
            def ssim():
                rc = lib.srk_ssim(ptr(pd), _strides4(pd), ptr(gd), _strides4(gd), 1, c, H, W, 0, SSIM_DOMAINS[domain],
                                  ptr(out[0:1]), ptr(out[1:2]), ptr(out[2:3]), ptr(ws), stream_ptr())
                assert rc == 0
            med, lo = _events(ssim)
            got = [float(v) for v in out.cpu()]
            print("  srk_ssim %-6s (ssim+psnr+mse) median %8.1f us  min %8.1f us  %5.1f %% of 8 TB/s   ssim %.6f psnr %.4f"
                  % (domain, med, lo, 100 * need / (med * 1e-6) / PEAK, got[0], got[1]))
        t0 = time.perf_counter()
        ph, gh = pd.cpu().numpy(), gd.cpu().numpy()
        t1 = time.perf_counter()
        want = ssim_ref.ssim_ref(ph, gh)
        t2 = time.perf_counter()
        lib.srk_ssim(ptr(pd), _strides4(pd), ptr(gd), _strides4(gd), 1, c, H, W, 0, 0, ptr(out[0:1]), ptr(out[1:2]),
                     ptr(out[2:3]), ptr(ws), stream_ptr())
        print("  host route: copy %.1f ms + numpy fp64 restatement %.1f ms; ssim %.9f, device 'float' off by %.2e"
              % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, want[0], abs(float(out[0]) - want[0])))


def resources():
    csrc = os.path.join(ROOT, "pytorch_super_resolution_model_collection_amd", "csrc")
    from pytorch_super_resolution_model_collection_amd import _build
    cmd = [_build._hipcc()] + _build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "ssim.hip"),
                                             "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    for line in r.stderr.splitlines():
        if "remark:" in line and any(k in line for k in ("Function Name", "VGPRs:", "SGPRs:", "ScratchSize", "Occupancy",
                                                         "LDS Size")):
            print(line.split("remark:")[1].replace("[-Rpass-analysis=kernel-resource-usage]", "").rstrip())


if __name__ == "__main__":
    {"time": timing, "resources": resources}[sys.argv[1] if len(sys.argv) > 1 else "time"]()
