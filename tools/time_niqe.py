#!/usr/bin/env python3
"""Evidence for DESIGN 34 (NIQE features on the device), run from the repo root on the MI355X box:

  python tools/time_niqe.py [--quick]

Times ops.niqe_features (k_niqe_scale<1> + k_niqe_scale<2>, two launches) on a float NCHW picture of [3, 512, 512] and
[3, 1356, 2040], block 96, by HIP events, warm, in five rounds that alternate with a torch composition of the same
arithmetic on the device (fp64 conv2d windows, unfold blocks, masked sums, argmin over the table); the scipy restatement of
tests/niqe_ref.py on the CPU is timed once per size beside them.  Then the cost of test() per picture with and without
--niqe_params on a synthetic loader (ESPCN x4, four pictures of 120 x 120 -> 448 x 448), host clock around a synchronise,
five alternating rounds.

"HBM floor" is the bytes the algorithm needs -- the picture once, P_2 (fp64, a quarter of the crop) written and read --
over 8 TB/s; the share is that time over the measured one."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK, ROUNDS, BLOCK = 8e12, 5, 96
SIZES = ((512, 512), (1356, 2040))


def _events(fn, reps):
    import torch
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return statistics.median(us)


def torch_features(img, block, tables, window):
    """The definition of include/srk.h composed from torch operators on the device, fp64; img: [3, H, W] float in [0, 1]."""
    import torch
    import torch.nn.functional as F
    import niqe_ref as R
    b8 = (img.clamp(0, 1) * 255.0).to(torch.uint8).double()
    P = torch.round(16.0 + (65.481 * b8[0] + 128.553 * b8[1] + 24.966 * b8[2]) / 255.0)
    nh, nw = P.shape[0] // block, P.shape[1] // block
    P = P[:nh * block, :nw * block]
    shrink = torch.tensor(R.SHRINK, device=img.device)
    gam = torch.tensor(R.GAM, device=img.device)
    out = []
    for b in (block, block // 2):
        def win(x):
            x = F.pad(x[None, None], (3, 3, 3, 3), mode='replicate')
            return F.conv2d(F.conv2d(x, window.view(1, 1, 1, 7)), window.view(1, 1, 7, 1))[0, 0]
        mu = win(P)
        sigma = (win(P * P) - mu * mu).abs().sqrt()
        n = (P - mu) / (sigma + 1.0)
        B = n.unfold(0, b, b).unfold(1, b, b).reshape(nh * nw, b, b)
        feats = []
        for k, shift in enumerate(((0, 0),) + R.SHIFTS):
            m = (B if k == 0 else B * torch.roll(B, shift, dims=(1, 2))).reshape(nh * nw, -1)
            neg, pos, m2 = m < 0, m > 0, m * m
            cn, cp = neg.sum(1).double(), pos.sum(1).double()
            ls, rs = ((m2 * neg).sum(1) / cn).sqrt(), ((m2 * pos).sum(1) / cp).sqrt()
            gh = ls / rs
            q = m2.sum(1)
            rhat = (m.abs().sum(1) / m.shape[1]) ** 2 / (q / m.shape[1])
            rn = rhat * (gh ** 3 + 1) * (gh + 1) / (gh ** 2 + 1) ** 2
            j = ((tables[0][None, :] - rn[:, None]) ** 2).argmin(1)
            bad = (cn == 0) | (cp == 0) | (q == 0)
            nan = torch.full_like(rn, float('nan'))
            alpha, bl, br = gam[j], ls * tables[1][j], rs * tables[1][j]
            cols = [alpha, (bl + br) / 2] if k == 0 else [alpha, (br - bl) * tables[2][j], bl, br]
            feats += [torch.where(bad, nan, c) for c in cols]
        out.append(torch.stack(feats, 1))
        if b == block:
            h, w = P.shape
            ar = torch.arange(8, device=img.device)
            rows = 2 * torch.arange(h // 2, device=img.device)[:, None] - 3 + ar[None]
            rows = torch.where(rows < 0, -rows - 1, rows)
            rows = torch.where(rows >= h, 2 * h - 1 - rows, rows)
            v = torch.einsum('k,ikx->ix', shrink, P[rows])
            cols = 2 * torch.arange(w // 2, device=img.device)[:, None] - 3 + ar[None]
            cols = torch.where(cols < 0, -cols - 1, cols)
            cols = torch.where(cols >= w, 2 * w - 1 - cols, cols)
            P = torch.einsum('k,ijk->ij', shrink, v[:, cols])
    return torch.cat(out, 1)


def main():
    import numpy as np
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    import niqe_ref as R
    quick = "--quick" in sys.argv
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(0))
    tables = pkg.ops.niqe_tables(dev)
    window = torch.tensor(R.window(), device=dev)
    for h, w in SIZES[:1] if quick else SIZES:
        u8 = R.picture(7, 3, h, w)
        img = torch.from_numpy(u8.astype(np.float32) / np.float32(255)).to(dev)
        nh, nw = h // BLOCK, w // BLOCK
        need = 3 * 4 * h * w + 2 * 8 * (nh * BLOCK // 2) * (nw * BLOCK // 2)
        floor_us = need / PEAK * 1e6
        got = pkg.ops.niqe_features(img, 0, BLOCK)
        alt = torch_features(img, BLOCK, tables, window)
        t0 = time.perf_counter()
        ref = R.features(u8, 0, BLOCK)
        cpu_s = time.perf_counter() - t0
        ok = ~np.isnan(ref)
        print("\n[3, %d, %d] float NCHW, block %d: %d x %d blocks; bytes needed %.1f MB, HBM floor %.1f us"
              % (h, w, BLOCK, nh, nw, need / 1e6, floor_us))
        print("  kernels vs restatement: worst |d| / max(1, |ref|) %.2e;  torch composition vs restatement: %.2e"
              % (float((np.abs(got.cpu().numpy() - ref)[ok] / np.maximum(1, np.abs(ref[ok]))).max()),
                 float((np.abs(alt.cpu().numpy() - ref)[ok] / np.maximum(1, np.abs(ref[ok]))).max())))
        kern, comp = [], []
        for _ in range(ROUNDS):
            kern.append(_events(lambda: pkg.ops.niqe_features(img, 0, BLOCK), 10))
            comp.append(_events(lambda: torch_features(img, BLOCK, tables, window), 3))
        km, cm = statistics.median(kern), statistics.median(comp)
        print("  ops.niqe_features (2 launches)  median %9.1f us  (rounds %.1f .. %.1f)  %5.2f %% of the HBM floor's rate"
              % (km, min(kern), max(kern), 100 * floor_us / km))
        print("  torch composition on the device median %9.1f us  (rounds %.1f .. %.1f)  %.2fx the kernels"
              % (cm, min(comp), max(comp), cm / km))
        print("  scipy restatement on the CPU    one run %9.1f ms  %.0fx the kernels" % (cpu_s * 1e3, cpu_s * 1e6 / km))

    # test() with and without --niqe_params
    import main as cli
    from pytorch_super_resolution_model_collection_amd.sr_trainers import TRAINERS
    import tempfile
    tmp = tempfile.mkdtemp()
    mu_p, cov_p, _ = R.fitted_params()
    params = os.path.join(tmp, "p.npz")
    pkg.utils.save_niqe_params(params, mu_p, cov_p)
    base = ["--model_name", "ESPCN", "--num_channels", "3", "--scale_factor", "4", "--synthetic", "--save_dir", tmp]
    g = torch.Generator().manual_seed(5)
    loader = [(torch.rand(1, 3, 120, 120, generator=g), torch.rand(1, 3, 448, 448, generator=g)) for _ in range(4)]
    trainers = []
    for extra in ([], ["--niqe_params", params]):
        t = TRAINERS["ESPCN"](cli.parse_args(base + extra))
        t.model = t.build_model().to(t.device).eval()
        t.test(loader)
        trainers.append(t)
    times = ([], [])
    for _ in range(ROUNDS):
        for t, into in zip(trainers, times):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.test(loader)
            torch.cuda.synchronize()
            into.append((time.perf_counter() - t0) / len(loader) * 1e3)
    off, on = statistics.median(times[0]), statistics.median(times[1])
    print("\ntest() per picture (ESPCN x4, 120 x 120 -> 448 x 448, 4 x 4 blocks): without --niqe_params %.2f ms (rounds %.2f .. "
          "%.2f), with %.2f ms (rounds %.2f .. %.2f): + %.2f ms a picture (features on the device, finish on the host)"
          % (off, min(times[0]), max(times[0]), on, min(times[1]), max(times[1]), on - off))


if __name__ == "__main__":
    main()
