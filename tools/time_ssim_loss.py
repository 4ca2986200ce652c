#!/usr/bin/env python3
"""Evidence for DESIGN 20 (the SSIM training loss), run on the MI355X box from the repo root:

  python tools/time_ssim_loss.py kernel   ops.ssim_loss forward + backward (k_ssim_loss + k_ssim_loss_final, the backward
                                          seeded with the unit seed: no further launch) against the grouped-conv2d-plus-
                                          autograd torch composition of the same definition on the device, at
                                          [128, 3, 128, 128] (c4's HR batch), [256, 1, 41, 41] (c3) and [16, 3, 128, 128]
  python tools/time_ssim_loss.py step     one replayed EDSR x4 train step at c4's shape (128 LR patches of 32 x 32, Adam,
                                          L1) with --ssim_weight 0 and 0.16
  python tools/time_ssim_loss.py parity   the kernel against fp64 torch autograd on the case table of the tests: loss
                                          error, worst gradient error over the bar 1e-4 * max |ref| + 1e-9

HIP events; medians over five alternating rounds of 30 timed calls (steps: 20) each, with the spread of the round medians."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((128, 3, 128, 128), (256, 1, 41, 41), (16, 3, 128, 128))
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _events(fn, inner, warm=3):
    """ms per call: `inner` calls between two events"""
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _compare(sides, inner, rounds=5):
    """{name: fn} -> {name: (median, min, max of the round medians) ms per call}, the sides alternated"""
    res = {k: [] for k in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            res[name].append(_events(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


def torch_composition(dev):
    """1 - mean SSIM of an unclamped prediction with grouped F.conv2d (separable 11-tap passes) under autograd, fp32."""
    import torch
    import torch.nn.functional as F
    import ssim_ref
    g = torch.from_numpy(ssim_ref.window()).float().to(dev)

    def filt(a, c):
        a = F.conv2d(a, g.view(1, 1, 1, 11).expand(c, 1, 1, 11), groups=c)
        return F.conv2d(a, g.view(1, 1, 11, 1).expand(c, 1, 11, 1), groups=c)

    def loss(x, y):
        c = x.shape[1]
        mx, my = filt(x, c), filt(y, c)
        vx, vy, cov = filt(x * x, c) - mx * mx, filt(y * y, c) - my * my, filt(x * y, c) - mx * my
        s = ((2 * mx * my + C1) * (2 * cov + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
        return 1 - s.mean()
    return loss


def kernel():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    from pytorch_super_resolution_model_collection_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(5)
    composed = torch_composition(dev)
    for shape in SHAPES:
        t = torch.rand(shape, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
        x = (t + 0.05 * torch.randn(shape, generator=gen).to(dev)).contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)

        def fused():
            x.grad = None
            ops.backward(ops.ssim_loss(x, t))

        def torch_side():
            x.grad = None
            composed(x, t).backward()

        def forward_only():
            with torch.no_grad():
                ops.ssim_loss(x, t)
        fused()
        a, ga = float(ops.ssim_loss(x, t).detach()), x.grad.clone()
        torch_side()
        b, gb = float(composed(x, t).detach()), x.grad.clone()
        r = _compare({"kernel": fused, "torch": torch_side, "kernel, loss only": forward_only}, 30)
        k, tc, fo = r["kernel"], r["torch"], r["kernel, loss only"]
        print("%-20s k_ssim_loss fwd+bwd %8.3f ms (rounds %.3f .. %.3f), loss only %8.3f ms | torch composition fwd+bwd %8.3f ms "
              "(rounds %.3f .. %.3f) = %.2f x the kernel | loss %.7f vs %.7f, gradients differ by %.2e of their maximum"
              % ("x".join(str(v) for v in shape), k[0], k[1], k[2], fo[0], tc[0], tc[1], tc[2], tc[0] / k[0], a, b,
                 float((ga - gb).abs().max() / gb.abs().max())), flush=True)
        del x, t, ga, gb
        torch.cuda.empty_cache()


def step():
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import pytorch_super_resolution_model_collection_amd as pkg
    from oracle import fill
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(9)
    inp, tgt = torch.rand((128, 3, 32, 32), generator=gen).to(dev), torch.rand((128, 3, 128, 128), generator=gen).to(dev)
    steps = {}
    for a in (0.0, 0.16):
        net = pkg.EDSRNet(3, 64, 16)
        fill.fill_module(net, 3, 0.5)
        net.to(dev).train()
        flat, opt, dp, eager = pkg.trainers.build("edsr", net, 1e-5, ssim_weight=a)
        g = pkg.trainers.capture_step(eager, (inp, tgt), warmup=2, flats=[flat])
        steps[a] = (g, net, opt)
    r = _compare({a: (lambda s=s: s[0](*s[0].static)) for a, s in steps.items()}, 20)
    base, mix = r[0.0], r[0.16]
    print("EDSR x4 step, 128 x 3 x 32 x 32 -> 128 x 128, replayed graph: --ssim_weight 0 %8.3f ms (rounds %.3f .. %.3f) | "
          "--ssim_weight 0.16 %8.3f ms (rounds %.3f .. %.3f) | the loss adds %.3f ms = %.2f %%"
          % (base[0], base[1], base[2], mix[0], mix[1], mix[2], mix[0] - base[0], (mix[0] / base[0] - 1) * 100), flush=True)
    torch.cuda.synchronize()
    for s in steps.values():
        s[0].close()


def parity():
    import numpy as np
    import torch
    import __graft_entry__
    __graft_entry__.build()
    import ssim_loss_ref as L
    from pytorch_super_resolution_model_collection_amd import ops
    dev = torch.device("cuda", 0)
    for name in sorted(L.cases()):
        p, g = L.cases()[name]
        want_loss, want_grad = L.reference(name)
        x = torch.from_numpy(p).to(dev).requires_grad_(True)
        loss = ops.ssim_loss(x, torch.from_numpy(g).to(dev))
        ops.backward(loss)
        err = float(np.abs(x.grad.cpu().numpy().astype(np.float64) - want_grad).max())
        ref = float(np.abs(want_grad).max())
        print("%-14s loss off by %.2e | gradient: worst |d| %.3e, max |ref| %.3e, %.4f of the bar"
              % (name, abs(float(loss) - want_loss), err, ref, err / (1e-4 * ref + 1e-9)), flush=True)


if __name__ == "__main__":
    {"kernel": kernel, "step": step, "parity": parity}[sys.argv[1]]()
